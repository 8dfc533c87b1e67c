"""DecodeOptions: the per-pass decode options as one frozen record, normalised and checked once."""
import dataclasses

import pytest

from twamd import seqbias
from twamd.engine import NO_OPTIONS, DecodeOptions

V, EOS = 1000, 999


def test_none_and_neutral_values_are_one_record_without_a_pre_pass():
    off = DecodeOptions.make(V, EOS)
    same = [DecodeOptions.make(V, EOS, repetition_penalty=None, no_repeat_ngram_size=None, length_penalty=None,
                               token_logprobs=None, sequence_bias=None, bad_words_ids=None),
            DecodeOptions.make(V, EOS, repetition_penalty=1.0, no_repeat_ngram_size=0, length_penalty=1.0,
                               token_logprobs=False),
            DecodeOptions.make(), DecodeOptions(), NO_OPTIONS]
    for o in same:
        assert o == off and hash(o) == hash(off) and not o.history and o.graph_key == off.graph_key
    assert (off.repetition_penalty, off.no_repeat_ngram_size, off.length_penalty, off.token_logprobs) == (1.0, 0, 1.0,
                                                                                                        False)
    assert off.pre == () and off.post == () and off.hist_key == (1.0, 0, 0, 0)
    # bad_words_ids that only names the EOS leaves nothing to forbid: no entries, no pre-pass
    assert not DecodeOptions.make(V, EOS, bad_words_ids=[[EOS]]).history
    with pytest.raises(dataclasses.FrozenInstanceError):
        off.repetition_penalty = 1.3


def test_keys_separate_what_a_launch_or_a_captured_graph_bakes_in():
    mk = lambda **kw: DecodeOptions.make(V, EOS, **kw)  # noqa: E731
    one, two = mk(sequence_bias={(5,): 1.0}), mk(sequence_bias={(5,): 1.0, (6, 7): -1.0})
    bad = mk(bad_words_ids=[[5]])
    assert one.hist_key == (1.0, 0, 1, 0) and two.hist_key == (1.0, 0, 2, 0) and bad.hist_key == (1.0, 0, 0, 1)
    assert all(o.history for o in (one, two, bad))
    pen, ngram = mk(repetition_penalty=1.3), mk(no_repeat_ngram_size=2)
    assert pen.hist_key == (1.3, 0, 0, 0) and ngram.hist_key == (1.0, 2, 0, 0) and pen.history and ngram.history
    keys = [o.graph_key for o in (mk(), one, two, bad, pen, ngram, mk(repetition_penalty=1.5))]
    assert len(set(keys)) == len(keys)
    # the log-probability flag runs no pre-pass and changes no history key, but a captured step differs by it
    lp = mk(token_logprobs=True)
    assert not lp.history and lp.hist_key == mk().hist_key and lp.graph_key != mk().graph_key and lp != mk()
    assert mk(repetition_penalty=1.3, token_logprobs=True).graph_key != pen.graph_key
    # the table's contents and the beam exponent ride elsewhere (the table buffers, the beam graph's own key)
    assert mk(sequence_bias={(8,): 2.0}).graph_key == one.graph_key and mk(sequence_bias={(8,): 2.0}) != one
    assert mk(length_penalty=0.5).graph_key == mk().graph_key and mk(length_penalty=0.5).length_penalty == 0.5


def test_entries_are_the_checked_ones_in_table_order():
    sb = [[[5, 6], -2.0], [[7], 1.5], [[5, 6], 3.0]]
    bw = [[8, 9], [EOS], [4], [8, 9]]
    o = DecodeOptions.make(V, EOS, sequence_bias=sb, bad_words_ids=bw)
    assert o.pre == tuple(seqbias.sequence_bias_entries(sb, V)) == (((7,), 1.5), ((5, 6), 3.0))
    assert o.post == tuple(seqbias.bad_words_entries(bw, EOS, V)) == (((4,), float("-inf")), ((8, 9), float("-inf")))
    assert hash(o) == hash(DecodeOptions.make(V, EOS, sequence_bias={(7,): 1.5, (5, 6): 3.0}, bad_words_ids=[[4], [8, 9]]))


@pytest.mark.parametrize("kw, fn", [
    ({"sequence_bias": {}}, lambda: seqbias.sequence_bias_entries({}, V)),
    ({"sequence_bias": {(1, 2): 1}}, lambda: seqbias.sequence_bias_entries({(1, 2): 1}, V)),
    ({"sequence_bias": {(1, V): 1.0}}, lambda: seqbias.sequence_bias_entries({(1, V): 1.0}, V)),
    ({"bad_words_ids": []}, lambda: seqbias.bad_words_entries([], EOS, V)),
    ({"bad_words_ids": [[1, -2]]}, lambda: seqbias.bad_words_entries([[1, -2]], EOS, V)),
    ({"bad_words_ids": [[]]}, lambda: seqbias.bad_words_entries([[]], EOS, V)),
    ({"bad_words_ids": [[V + 3]]}, lambda: seqbias.bad_words_entries([[V + 3]], EOS, V)),
    ({"sequence_bias": {(i + 1,): 1.0 for i in range(200)}, "bad_words_ids": [[i + 1] for i in range(57)]},
     lambda: seqbias.check_limits([((1,), 1.0)] * 200, [((1,), 0.0)] * 57)),
    ({"sequence_bias": {tuple(range(1, 18)): 1.0}}, lambda: seqbias.check_limits([(tuple(range(1, 18)), 1.0)], [])),
])
def test_invalid_entries_raise_seqbias_messages_from_the_constructor(kw, fn):
    with pytest.raises(ValueError) as theirs:
        fn()
    with pytest.raises(ValueError) as ours:
        DecodeOptions.make(V, EOS, **kw)
    assert str(ours.value) == str(theirs.value)


def test_limits_are_inclusive():
    o = DecodeOptions.make(V, EOS, sequence_bias={(i + 1,): 1.0 for i in range(200)},
                           bad_words_ids=[[i + 1] for i in range(56)], )
    assert o.hist_key == (1.0, 0, 200, 56)
    assert DecodeOptions.make(V, EOS, sequence_bias={tuple(range(1, 17)): 1.0}).history


def test_unknown_keyword_raises_type_error():
    with pytest.raises(TypeError, match="top_p"):
        DecodeOptions.make(V, EOS, top_p=0.9)
    with pytest.raises(TypeError):
        DecodeOptions.make(V, EOS, 1.3)  # (the options are keywords)
