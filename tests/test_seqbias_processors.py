"""sequence_bias / bad_words_ids without a GPU: the numpy restatement (tests/seqbias_ref.py) equals transformers'
SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor bit for bit, alone and chained with the penalty and n-gram
processors in _get_logits_processor's order; the callable and the engine validate the options with transformers' messages and
order them as the kernel's table; and the new kernel's symbol, ctypes signature, struct and torch op are there."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import history_ref as hr
import seqbias_ref as sr
from test_history_processors import kernel_logits
from twamd import _lib, _ops, seqbias
from twamd.config import PRESETS
from twamd.pipeline import TurboTranscriber

V = PRESETS["test-mini"].vocab
EOS = 50257
LANG = 50262  # the id the rows' TW_HIST_LANG slot stands for
LONG = list(range(101, 117))  # an entry of TW_SEQBIAS_MAX_IDS ids
TINY = float(2.0 ** -24)  # 1.0 + TINY == 1.0 in f32, TINY + TINY + 1.0 != 1.0: the sum's order shows
# (penalty, n-gram size) of the chained runs
CHAINS = ((1.0, 0), (1.3, 2), (0.7, 3))

# sequence_bias in the kernel's table order (1-id entries first)
PRE = [
    ((500,), 1.0),            # 1-id entry on the id three longer entries end in
    ((7,), float("-inf")),    # -inf in the pre stage
    ((50364,), 5.0),          # a positive bias onto a logit that is already -inf (rows 1..)
    ((31, 1234, 500), TINY),  # the entry the history lengths go around (3 ids)
    ((1234, 500), TINY),      # ends in the same id: fires with the one above on ... 31 1234
    ((0, 500), 3.0),          # ends in the same id, does not fire
    (tuple(LONG), 2.0),       # the maximum id count; fires on row 5 across the boundary and through the language slot
    ((LONG[13], LONG[14], 950), -2.5),  # fires on row 5 inside the generated tokens
    ((LONG[4], LONG[5], 951), 1.5),     # a tail that row 5 holds earlier, not at its end: does not fire
    ((31, 1234, 960), 7.0),   # 3 ids on an id of its own: skipped on row 2 (one longer than [31 1234]), fires on 3, 4
]
# bad_words_ids
POST = [
    [50365],
    [1234, 9],    # rows 3 and 4 hold 9: the penalty touches it; row 4's 2-gram ban forbids it as well
    [1234, 500],  # an id the pre stage biased
    [31, 1234, 9, 9],  # longer than rows 2 and 3, does not fire on row 4
]
POST_ENTRIES = [(tuple(w), float("-inf")) for w in POST]


def seqbias_rows():
    """(prefix, generated, language slot index or None) of the six rows: history lengths 0, 1 and 2, 3, 4 around the
    3-id entry (2: the entry is one longer than the history and must not fire although its prefix fits), and a row of
    17 ids whose prefix / generated boundary and language slot lie inside the 16-id entry's match."""
    return [
        ([], [], None),
        ([1234], [], None),
        ([31], [1234], None),
        ([9, 31], [1234], None),
        ([1234, 9, 31], [1234], None),
        ([900, 901, LONG[0], LONG[1], LONG[2]], LONG[3:15], 3),
    ]


def row_history(row):
    pre, gen, _ = row
    return list(pre) + list(gen)


def seqbias_logits(R, ld):
    """kernel_logits without its -0.0 column (see seqbias_ref: the one value a dense add would change)."""
    x = kernel_logits(R, ld)
    x[:, 31] = np.float32(-0.75)
    x[3:, 9] = np.float32(4.0)
    assert not np.any((x == 0) & np.signbit(x))
    return x


def _tf_chain(x_row, history, pre, p, n, post):
    from transformers.generation.logits_process import (NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor)

    s = torch.from_numpy(x_row[None].copy())
    ids = torch.tensor([history], dtype=torch.long)
    if pre:
        s = SequenceBiasLogitsProcessor(sequence_bias=dict(pre))(ids, s)
    if p != 1.0 and history:
        s = RepetitionPenaltyLogitsProcessor(penalty=p)(ids, s)
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(n)(ids, s)
    if post:
        s = NoBadWordsLogitsProcessor([list(w) for w in post], eos_token_id=EOS)(ids, s)
    return s[0].numpy()


def test_restatement_equals_transformers_processors():
    pytest.importorskip("transformers")
    rows = seqbias_rows()
    x = seqbias_logits(len(rows), V)
    fired = set()
    for p, n in CHAINS:
        for pre, post in ((PRE, POST), (PRE, []), ([], POST)):
            for r, row in enumerate(rows):
                h = row_history(row)
                ref = sr.chain(x[r], h, pre, p, n, [(tuple(w), float("-inf")) for w in post])
                got = _tf_chain(x[r], h, pre, p, n, post)
                assert ref.dtype == np.float32
                assert np.array_equal(got.view(np.int32), ref.view(np.int32)), (p, n, r, bool(pre), bool(post))
                fired |= {(r, e) for e, (ids, _) in enumerate(PRE) if len(ids) > 1 and sr.fires(ids, h)}
    # the cases the rows are there for
    assert (2, 3) not in fired and (3, 3) in fired and (4, 3) in fired  # len == L + 1 skipped; L and L + 1 fire
    assert (1, 4) not in fired and (3, 4) in fired and (5, 6) in fired and (5, 7) in fired and (5, 8) not in fired
    assert not any(e == 5 for _, e in fired)
    assert {r for r, e in fired if e == 9} == {3, 4}


def test_sum_order_is_transformers_and_shows():
    """Row 3: the 1-id entry and two longer ones end in id 500. transformers' order gives x + 1.0; adding the two
    small biases first would give x + (1 + 2^-23)."""
    pytest.importorskip("transformers")
    rows = seqbias_rows()
    x = seqbias_logits(len(rows), V)
    h = row_history(rows[3])
    got = _tf_chain(x[3], h, PRE, 1.0, 0, [])
    assert got[500] == np.float32(x[3, 500] + np.float32(1.0))
    other = np.float32(x[3, 500] + np.float32(np.float32(TINY) + np.float32(TINY) + np.float32(1.0)))
    assert other != got[500]
    assert sr.sequence_bias(x[3], h, PRE)[500] == got[500]
    # the callable's ordering: whatever the dict's order, 1-id entries come first and the rest keep their order
    shuffled = {ids: b for ids, b in (PRE[3], PRE[0], PRE[6], PRE[4], PRE[1], PRE[9], PRE[5], PRE[2], PRE[7], PRE[8])}
    ent = seqbias.sequence_bias_entries(shuffled, V)
    assert [ids for ids, _ in ent] == [PRE[0][0], PRE[1][0], PRE[2][0], PRE[3][0], PRE[6][0], PRE[4][0], PRE[9][0],
                                       PRE[5][0], PRE[7][0], PRE[8][0]]
    ref = _tf_chain(x[3], h, list(shuffled.items()), 1.0, 0, [])
    assert np.array_equal(sr.sequence_bias(x[3], h, ent).view(np.int32), ref.view(np.int32))


def test_zero_sign_is_the_only_difference_from_a_dense_add():
    pytest.importorskip("transformers")
    x = kernel_logits(6, V)  # (column 31 is -0.0)
    h = row_history(seqbias_rows()[3])
    got, ref = _tf_chain(x[3], h, PRE, 1.0, 0, []), sr.sequence_bias(x[3], h, PRE)
    diff = np.flatnonzero(got.view(np.int32) != ref.view(np.int32))
    assert diff.tolist() == [31] and got[31] == 0 and ref[31] == 0
    assert np.array_equal(got, ref)


def test_restatement_properties():
    x = np.array([1.0, 2.0, -np.inf, 0.5, 3.0], np.float32)
    assert sr.fires([4], []) and not sr.fires([1, 2], [1]) and sr.fires([1, 2], [0, 1]) and not sr.fires([1, 2], [1, 0])
    assert not sr.fires([0, 1, 2], [0, 1])  # len == L + 1: skipped although its prefix fits
    s = sr.sequence_bias(x, [0, 1], [((3,), 2.0), ((1, 3), 0.25), ((0, 3), 8.0), ((1, 2), 5.0)])
    assert s[3] == np.float32(2.75) and np.isneginf(s[2]) and s[0] == x[0]
    assert np.isneginf(sr.bad_words(x, [0, 1], [[1, 4], [0]])[[0, 4]]).all()
    # order of the stages: the bias decides the sign the penalty sees; a bad word wins over everything
    both = sr.chain(x, [3], [((3,), -1.0)], 2.0, 0, [])
    assert both[3] == np.float32(-0.5) * np.float32(2.0)
    assert np.isneginf(sr.chain(x, [0, 3], [((3,), 9.0)], 2.0, 0, [((3, 1), float("-inf"))])[1])
    assert np.array_equal(sr.chain(x, [0, 1, 0], (), 1.3, 2, ()), hr.history_processors(x, [0, 1, 0], 1.3, 2))


def _bad_words(bw, vocab=None, eos=None):
    """What WhisperEngine.generate makes of bad_words_ids (twamd.seqbias): the checked -inf entries in table order."""
    ent = seqbias.bad_words_entries(bw, eos, vocab)
    seqbias.check_limits([], ent)
    return [list(ids) for ids, _ in ent]


def test_callable_pops_orders_and_limits():
    """The callable takes sequence_bias; bad_words_ids stays in generate_kwargs (the callable goes on refusing it:
    tests/test_gpu_penalties.py), the engine's generate() takes it through the same module."""
    pop = TurboTranscriber._history_options
    assert pop({"sequence_bias": None}) == {}
    gk = {"sequence_bias": [[[5, 6], -2.0], [[7], 1.5], [[5, 6], 3.0]], "bad_words_ids": [[8, 9]],
          "repetition_penalty": 1.3, "top_p": 0.9}
    out = pop(gk, vocab=V)
    assert gk == {"top_p": 0.9, "bad_words_ids": [[8, 9]]}
    assert list(out["sequence_bias"].items()) == [((7,), 1.5), ((5, 6), 3.0)]  # (a repeated key takes its last bias)
    assert out["repetition_penalty"] == 1.3 and "bad_words_ids" not in out
    assert pop({"sequence_bias": {(3, 4): 1.0, (2,): -1.0}}) == {"sequence_bias": {(2,): -1.0, (3, 4): 1.0}}
    assert list(pop({"sequence_bias": {(3, 4): 1.0, (2,): -1.0}})["sequence_bias"]) == [(2,), (3, 4)]
    # what comes back passes the same checks again (the engine repeats them)
    assert pop(dict(out), vocab=V) == out
    assert _bad_words([[8, 9], [EOS], [4], [8, 9]], V, EOS) == [[4], [8, 9]]
    with pytest.raises(ValueError, match="at most 256"):
        _bad_words([[i + 1] for i in range(257)])
    assert len(_bad_words([[i + 1] for i in range(256)])) == 256
    with pytest.raises(ValueError, match="at most 256"):
        pop({"sequence_bias": {(i + 1,): 1.0 for i in range(257)}})
    with pytest.raises(ValueError, match="at most 16 per entry"):
        pop({"sequence_bias": {tuple(range(1, 18)): 1.0}})
    assert pop({"sequence_bias": {tuple(range(1, 17)): 1.0}})


def test_minus_inf_bias_forbids_like_a_bad_word():
    """What the callable offers instead of bad_words_ids: the same sequences as sequence_bias entries of -inf give
    the same scores bit for bit, in the restatement and in transformers, under every chain (-inf stays -inf through
    the penalty and the n-gram stage; a finite bias on the same sequence is overruled either way)."""
    pytest.importorskip("transformers")
    rows = seqbias_rows()
    x = seqbias_logits(len(rows), V)
    merged = dict(PRE)
    merged.update(POST_ENTRIES)
    merged = seqbias.sequence_bias_entries(merged, V)
    for p, n in CHAINS:
        for r, row in enumerate(rows):
            h = row_history(row)
            want = _tf_chain(x[r], h, PRE, p, n, POST)
            assert np.array_equal(sr.chain(x[r], h, merged, p, n, []).view(np.int32), want.view(np.int32)), (p, n, r)
            assert np.array_equal(_tf_chain(x[r], h, merged, p, n, []).view(np.int32), want.view(np.int32)), (p, n, r)


BAD_SEQUENCE_BIAS = [{}, [], "x", {(1, 2): 1}, {(1, 2): "a"}, {[1][0]: 1.0}, {(): 1.0}, {(1, -2): 1.0}, {(1, 2.0): 1.0},
                     [[[1, 2], 1]], [[[0, 2], 1.0]], [[(1, 2), 1.0]], [[[1, -2], 1.0]]]
BAD_BAD_WORDS = [[], "x", {}, [[1], 2], [[1, -2]], [[1, 2.0]]]


def test_validation_text_is_transformers_own():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, SequenceBiasLogitsProcessor

    pop = TurboTranscriber._history_options
    for bad in BAD_SEQUENCE_BIAS:
        with pytest.raises(ValueError) as theirs:
            SequenceBiasLogitsProcessor(sequence_bias=bad)
        with pytest.raises(ValueError) as ours:
            pop({"sequence_bias": bad}, vocab=V)
        assert str(ours.value) == str(theirs.value), bad
    for bad in BAD_BAD_WORDS:
        with pytest.raises(ValueError) as theirs:
            NoBadWordsLogitsProcessor(bad, eos_token_id=EOS)
        with pytest.raises(ValueError) as ours:
            _bad_words(bad, V, EOS)
        assert str(ours.value) == str(theirs.value), bad
    # ids past the vocabulary: transformers raises at the first call, the callable before any work
    x, ids = torch.zeros(1, V), torch.zeros(1, 3, dtype=torch.long)
    for key, bad, proc, ours_fn in (
            ("sequence_bias", {(1, V): 1.0, (V + 3,): 2.0}, lambda b: SequenceBiasLogitsProcessor(sequence_bias=b),
             lambda b: pop({"sequence_bias": b}, vocab=V)),
            ("bad_words_ids", [[1, V], [V + 3]], lambda b: NoBadWordsLogitsProcessor(b, EOS),
             lambda b: _bad_words(b, V, EOS))):
        with pytest.raises(ValueError) as theirs:
            proc(bad)(ids, x)
        with pytest.raises(ValueError) as ours:
            ours_fn(bad)
        assert str(ours.value) == str(theirs.value), key
    assert pop({"sequence_bias": {(V - 1,): 1.0}}, vocab=V)
    # [eos] alone is dropped, as transformers drops it: nothing is left to forbid. An empty sequence, which transformers
    # accepts and then fails on with an IndexError in its first call, is refused
    assert NoBadWordsLogitsProcessor([[EOS]], eos_token_id=EOS).sequence_bias == {}
    assert _bad_words([[EOS]], V, EOS) == []
    with pytest.raises(ValueError, match="non-empty"):
        _bad_words([[4], []], V, EOS)


def test_symbol_signature_struct_and_op():
    lib = _lib.load()
    assert "tw_logits_history_bias" in _lib.EXPORTED and "tw_logits_history_bias" in _lib._SIGS
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "tw_whisper.h")).read()
    assert re.search(r"^int\s+tw_logits_history_bias\s*\(", hdr, flags=re.M) and "typedef struct TwSeqBias" in hdr
    for name, val in (("TW_SEQBIAS_MAX_ENTRIES", _lib.TW_SEQBIAS_MAX_ENTRIES), ("TW_SEQBIAS_MAX_IDS",
                                                                               _lib.TW_SEQBIAS_MAX_IDS)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == val
    assert _lib.TW_SEQBIAS_MAX_ENTRIES >= 256 and _lib.TW_SEQBIAS_MAX_IDS >= 16
    assert (seqbias.MAX_ENTRIES, seqbias.MAX_IDS) == (_lib.TW_SEQBIAS_MAX_ENTRIES, _lib.TW_SEQBIAS_MAX_IDS)
    # tw_logits_history's arguments, then the table, then the stream
    a, b = _lib._SIGS["tw_logits_history"][0], _lib._SIGS["tw_logits_history_bias"][0]
    assert b[:len(a) - 1] == a[:-1] and len(b) == len(a) + 1 and b[-1] == a[-1]
    assert b[-2] is ctypes.POINTER(_lib.TwSeqBias)
    t = _lib.TwSeqBias
    assert [f for f, _ in t._fields_] == ["ids", "len", "bias", "ld_ids", "n_pre", "n_post"]
    assert (t.ld_ids.offset, t.n_pre.offset, t.n_post.offset, ctypes.sizeof(t)) == (24, 28, 32, 40)
    # argument errors are refused on the host, before any launch, with a message
    fn = lib.tw_logits_history_bias
    assert fn(None, 1, 8, 8, None, 0, None, None, 0, None, 1.3, 2, 0, None, None) != 0
    for table, word in ((t(1, 1, 1, 16, 200, 57), "TW_SEQBIAS_MAX_ENTRIES"), (t(1, 1, 1, 17, 1, 0), "ld_ids"),
                        (t(1, 1, 1, 16, -1, 2), "TW_SEQBIAS_MAX_ENTRIES"), (t(0, 1, 1, 16, 1, 0), "table arrays")):
        assert fn(1, 1, 8, 8, None, 0, None, 1, 0, 1, 1.0, 0, 0, ctypes.byref(table), None) != 0
        assert word in lib.tw_last_error().decode()
    tw = _ops.load()
    assert "logits_history_bias_" in _ops.OPS
    schema = str(tw.logits_history_bias_.default._schema)
    assert "Tensor(a!) logits" in schema and "Tensor bias_ids" in schema and "int n_post" in schema
    meta = torch.device("meta")
    x = torch.empty(2, 16, device=meta)
    i = torch.empty(2, 8, dtype=torch.int32, device=meta)
    assert tw.logits_history_bias_(x, 16, None, None, i, i, 1.3, 2, False, i, i[0], x[0], 1, 1) is None
