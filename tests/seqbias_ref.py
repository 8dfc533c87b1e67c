"""Numpy restatement of transformers' SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor
(generation/logits_process.py) for one row, and the full five-stage chain of tw_logits_history_bias:
(log_softmax) -> sequence bias -> repetition penalty -> no-repeat n-gram -> bad words. tests/test_seqbias_processors.py
pins it to transformers' own classes bit for bit; the GPU tests compare the kernel and the engine against it.

Entries are (ids, bias) pairs in the kernel's table order: 1-id entries first, then the longer ones in the dict's order
(twamd.seqbias does the ordering). The restatement adds the bias only at ids where an entry fires, as the kernel does;
transformers adds a dense bias vector to the whole row. The two agree bit for bit on every score except -0.0 at an id
no entry fires on, which transformers' `scores + 0.0` turns into +0.0 — an equal value that no later stage tells
apart (test_zero_sign_is_the_only_difference_from_a_dense_add)."""
from typing import Sequence, Tuple

import numpy as np

import history_ref as hr

Entry = Tuple[Sequence[int], float]


def fires(ids: Sequence[int], history: Sequence[int]) -> bool:
    """A 1-id entry always fires; a longer one when it is no longer than the history (transformers skips
    len(ids) > input_ids.shape[1], so len == L + 1 does not fire although its prefix would fit) and the history ends
    in its first len - 1 ids."""
    n = len(ids)
    if n == 1:
        return True
    if n == 0 or n > len(history):
        return False
    return [int(t) for t in history[len(history) - (n - 1):]] == [int(t) for t in ids[:-1]]


def sequence_bias(scores: np.ndarray, history: Sequence[int], entries: Sequence[Entry]) -> np.ndarray:
    """scores + bias, with bias built in f32 from 0.0 by adding the firing entries' biases in table order at their
    last ids (transformers: zeros, += length_1_bias, += every matching longer entry in dict order)."""
    s = np.array(scores, copy=True)
    total = {}
    for ids, b in entries:
        last = int(ids[-1])
        if 0 <= last < s.shape[0] and fires(ids, history):
            total[last] = np.float32(total.get(last, np.float32(0.0)) + np.float32(b))
    with np.errstate(invalid="ignore"):
        for last, t in total.items():
            s[last] = s[last] + s.dtype.type(t)
    return s


def bad_words(scores: np.ndarray, history: Sequence[int], words: Sequence[Sequence[int]]) -> np.ndarray:
    """NoBadWordsLogitsProcessor: the same processor with bias -inf for every sequence."""
    return sequence_bias(scores, history, [(list(w), float("-inf")) for w in words])


def chain(scores: np.ndarray, history: Sequence[int], pre: Sequence[Entry] = (), penalty: float = 1.0, ngram: int = 0,
          post: Sequence[Entry] = (), to_logprobs: bool = False) -> np.ndarray:
    """The five stages in _get_logits_processor's order (history_ref.history_processors with both tables empty).
    post: the bad words as (ids, -inf) entries, as the kernel's table holds them."""
    s = np.array(scores, copy=True)
    if to_logprobs:
        m = np.max(s)
        s = s - (m + np.log(np.sum(np.exp(s - m))))
    s = sequence_bias(s, history, pre)
    s = hr.history_processors(s, history, penalty, ngram)
    return sequence_bias(s, history, post)
