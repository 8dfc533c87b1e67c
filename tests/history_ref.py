"""Numpy restatement of transformers' RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor
(generation/logits_process.py) for one row: the reference of tw_logits_history. tests/test_history_processors.py pins it
to transformers' own classes bit for bit; the GPU tests compare the kernel and the engine against it."""
from typing import Sequence

import numpy as np


def repetition_penalty(scores: np.ndarray, history: Sequence[int], penalty: float) -> np.ndarray:
    """score = gather(scores, ids); where(score < 0, score * p, score / p); scatter — every value from the
    unpenalised row, so an id that occurs twice is penalised once. The arithmetic runs at the row's dtype."""
    s = np.array(scores, copy=True)
    if penalty == 1.0 or len(history) == 0:
        return s
    ids = np.unique(np.asarray(history, np.int64))
    p = s.dtype.type(penalty)
    old = s[ids]
    s[ids] = np.where(old < 0, old * p, old / p)
    return s


def banned_ngram_tokens(history: Sequence[int], n: int) -> list:
    """_calc_banned_ngram_tokens: the ids that followed an earlier occurrence of the history's last n - 1 ids."""
    h = [int(t) for t in history]
    L = len(h)
    if n <= 0 or L < n:  # (L + 1 < n in transformers: no n-gram can be completed; L == n - 1 has no earlier n-gram)
        return []
    tail = h[L - n + 1:]
    return sorted({h[i + n - 1] for i in range(L - n + 1) if h[i: i + n - 1] == tail})


def no_repeat_ngram(scores: np.ndarray, history: Sequence[int], n: int) -> np.ndarray:
    s = np.array(scores, copy=True)
    ban = banned_ngram_tokens(history, n)
    if ban:
        s[ban] = -np.inf
    return s


def history_processors(scores: np.ndarray, history: Sequence[int], penalty: float = 1.0, ngram: int = 0,
                       to_logprobs: bool = False) -> np.ndarray:
    """Penalty, then the bans (generate()'s order); to_logprobs: log_softmax first, as beam search scores rows (at the
    row's dtype: float64 rows give the float64 reference)."""
    s = np.array(scores, copy=True)
    if to_logprobs:
        m = np.max(s)
        s = s - (m + np.log(np.sum(np.exp(s - m))))
    return no_repeat_ngram(repetition_penalty(s, history, penalty), history, ngram)
