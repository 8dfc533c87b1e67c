"""Float64 restatement of the token alternatives (tw_token_topk): the k best eligible ids of one row's processed
scores with their log-probabilities. The scores are confidence_ref.step_logprobs' (oracle.whisper_oracle's processor
chain); eligible = finite after the processors (no text id when the timestamp rule fired); the ranking compares the
f32 scores, which are exact in float64, by (-score, id); lp = score - logsumexp(scores over the eligible set)."""
from typing import List, Sequence, Tuple

import numpy as np

import confidence_ref as cr
from oracle import whisper_oracle as wo


def rank(s: np.ndarray, k: int) -> Tuple[List[int], List[float]]:
    """The top k of processed scores s (f32 values, -inf where not eligible): ids by (-score, id) and their
    log-probabilities over the eligible set; shorter than k when fewer ids are eligible."""
    s = np.asarray(s, np.float64)
    ok = np.nonzero(np.isfinite(s))[0]
    order = ok[np.lexsort((ok, -s[ok]))][:k]
    lse = cr.logsumexp(s)
    return [int(i) for i in order], [float(s[i] - lse) for i in order]


def rule_margin(x: np.ndarray, sampled: Sequence[int], g) -> float:
    """logsumexp(timestamps) - max(text) of the scores before the timestamp rule (> 0: the rule fires)."""
    s = wo.process_logits_no_rule(np.asarray(x, np.float32), list(sampled), g).astype(np.float64)
    tb = g.ts_begin
    text = s[:tb][np.isfinite(s[:tb])]
    return float(cr.logsumexp(s[tb:]) - (text.max() if text.size else -np.inf))


def step_alternatives(x: np.ndarray, sampled: Sequence[int], g, use_ts: bool, k: int):
    """One step of one row: (ids, lps, margin). x f32[V] (already history-processed), sampled = the row's generated
    tokens so far; margin is the rule's (nan without timestamps)."""
    lp = cr.step_logprobs(x, sampled, g, use_ts)  # (log_softmax: a constant shift, the order is the scores')
    s = wo.process_logits(np.asarray(x, np.float32), list(sampled), g, use_ts)
    ids, _ = rank(s, k)
    return ids, [float(lp[i]) for i in ids], (rule_margin(x, sampled, g) if use_ts else float("nan"))


def raw_alternatives(x: np.ndarray, k: int):
    """No processor at all (forced alignment): the top k of log_softmax(x)."""
    return rank(np.asarray(x, np.float32), k)
