"""Numpy restatement of the per-token log-probability and of what the callable derives from it: the reference of
tw_token_logprob / tw_logits_sample_lp / tw_beam_step's fin_tlp and of twamd.tokenizer's word probability and
avg_logprob. lp = log_softmax(s)[token] with s the step's scores as generate() reports them (output_scores): the
processor chain of oracle.whisper_oracle.process_logits over the (already history-processed) row, in float64 past
the masks; the sum of a row's terms is what _retrieve_avg_logprobs averages."""
import math
from typing import List, Optional, Sequence

import numpy as np

from oracle import whisper_oracle as wo


def logsumexp(x: np.ndarray) -> float:
    x = np.asarray(x, np.float64)
    fin = x[np.isfinite(x)]
    if fin.size == 0:
        return -np.inf
    m = fin.max()
    return float(m + np.log(np.exp(fin - m).sum()))


def step_logprobs(x: np.ndarray, sampled: Sequence[int], g, use_ts: bool) -> np.ndarray:
    """log_softmax of one row's processed scores (f64; -inf where masked): x f32[V], sampled = the row's generated
    tokens so far."""
    s = wo.process_logits(np.asarray(x, np.float32), list(sampled), g, use_ts).astype(np.float64)
    return s - logsumexp(s)


def token_logprob(x: np.ndarray, sampled: Sequence[int], token: int, g, use_ts: bool) -> float:
    return float(step_logprobs(x, sampled, g, use_ts)[int(token)])


def topk_logprob(x: np.ndarray, token: int, top_k: int) -> float:
    """A sampled step without processors: x[token] - logsumexp(the top_k largest, ties at the k-th value kept) —
    the warped scores at temperature 1 (scores * T)."""
    x = np.asarray(x, np.float64)
    keep = x >= np.sort(x)[::-1][top_k - 1] if 0 < top_k < x.size else np.ones(x.size, bool)
    return float(x[int(token)] - logsumexp(x[keep]))


def word_probabilities(token_indices: Sequence[Sequence[int]], lps: Sequence[float]) -> List[float]:
    """openai-whisper's word probability: the arithmetic mean of exp(lp) over the word's tokens."""
    return [sum(math.exp(lps[k]) for k in ix) / len(ix) for ix in token_indices]


def mean_logprob(lps: Sequence[float]) -> Optional[float]:
    return sum(lps) / len(lps) if len(lps) else None


def lcs_cut_points(sequences: Sequence[Sequence[int]]) -> list:
    """The (lmid, rmid) cuts of tokenization_whisper._find_longest_common_sequence without timestamps (the
    sequential scan, restated independently of twamd.tokenizer): per junction, left keeps [:lmid], right [rmid:]."""
    cuts = []
    left = list(sequences[0])
    for right in sequences[1:]:
        ll, rl = len(left), len(right)
        best, best_idx = 0.0, (ll, ll, 0, 0)
        for i in range(1, ll + rl):
            ls, le = max(0, ll - i), min(ll, ll + rl - i)
            rs, re_ = max(0, i - ll), min(rl, i)
            matches = sum(1 for a, b in zip(left[ls:le], right[rs:re_]) if a == b)
            matching = matches / i + i / 10000.0
            if matches > 1 and matching > best:
                best, best_idx = matching, (ls, le, rs, re_)
        ls, le, rs, re_ = best_idx
        cuts.append(((le + ls) // 2, (re_ + rs) // 2))
        left = list(right[(re_ + rs) // 2:])
    return cuts
