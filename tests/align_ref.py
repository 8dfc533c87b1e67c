"""Reference of forced alignment (tw_logits_force, tw_align_cost, WhisperEngine.force_pass, TurboTranscriber.align),
composed at test time from oracle/whisper_oracle.py's primitives: the prompt and the given text ids go through
WhisperOracle.decoder_step with the cross-attention recording on, the log-probabilities are log_softmax of the
returned logits (raw: a forced pass chooses nothing, so no processor runs), and the times are
wo.token_timestamps over that one sequence — a row's own tokens and its own frame crop, nothing of a batch."""
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import whisper_oracle as wo


def log_softmax64(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def cost_matrix(w: np.ndarray, width: int = 7, dtype=np.float64) -> np.ndarray:
    """The DTW cost wo.token_timestamps builds from weights w [heads][rows][frames] that are already cropped and
    without prompt rows: -median_filter(standardised over the rows).mean(heads). dtype float32 is the oracle's own
    arithmetic (bit for bit), float64 the reference the GPU kernel is measured against."""
    w = np.asarray(w, dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = ((w - w.mean(axis=-2, keepdims=True)) / w.std(axis=-2, keepdims=True)).astype(dtype)
    return -wo.median_filter(z, width).mean(axis=0)


def times_from_cost(cost: np.ndarray, time_precision: float = 0.02) -> np.ndarray:
    """wo.token_timestamps' tail on a finished cost matrix [rows][frames]: f32 [rows + 1] seconds."""
    ti, tj = wo.dynamic_time_warping(np.asarray(cost, np.float64))
    jumps = np.pad(np.diff(ti), (1, 0), constant_values=1).astype(bool)
    jt = tj[jumps] * time_precision
    return np.concatenate([jt, [jt[-1]]]).astype(np.float32)


def forced_reference(model: "wo.WhisperOracle", enc: np.ndarray, prompt: Sequence[int], text_ids: Sequence[int],
                     eot: int, heads: Sequence[Tuple[int, int]], num_frames: Optional[int],
                     width: int = 7) -> Tuple[List[int], np.ndarray, np.ndarray]:
    """One window, teacher-forced: returns (tokens = text ids + EOT, their float64 log-probabilities, the token
    times in the engine's layout: len(prompt) zeros, then one time per token)."""
    P = len(prompt)
    toks = [int(t) for t in text_ids] + [int(eot)]
    fed = [int(t) for t in prompt] + toks[:-1]  # the EOT is scored, never fed
    cache = model.new_cache(enc)
    cache["xattn"] = {}
    lps = []
    for i, t in enumerate(fed):
        logits = model.decoder_step(t, cache)
        if i >= P - 1:  # the step that fed position i scores token i - (P - 1)
            lps.append(float(log_softmax64(logits)[toks[i - (P - 1)]]))
    x = cache["xattn"]
    w = np.stack([np.stack([x[t][l][h] for t in range(len(fed))]) for l, h in heads])
    return toks, np.asarray(lps, np.float64), wo.token_timestamps(w, P, num_frames, width)
