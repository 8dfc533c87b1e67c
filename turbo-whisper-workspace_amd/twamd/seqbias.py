"""generate()'s `sequence_bias` and `bad_words_ids` on the host: transformers' argument checks with its messages
(SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor._validate_arguments and the vocabulary check of
_prepare_bias_variables, generation/logits_process.py) and the entry table tw_logits_history_bias reads.

Table order: the sequence_bias entries first (1-id entries, then the longer ones, each group in the dict's order —
transformers adds length_1_bias before it walks the dict), then the bad_words_ids entries the same way with bias
-inf. Entries of one stage that end in the same id are summed by the kernel in this order."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

MAX_ENTRIES = 256  # TW_SEQBIAS_MAX_ENTRIES
MAX_IDS = 16       # TW_SEQBIAS_MAX_IDS

Entry = Tuple[Tuple[int, ...], float]


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer))


def validate_sequence_bias(sequence_bias: Any) -> None:
    """SequenceBiasLogitsProcessor._validate_arguments."""
    sb = sequence_bias
    if not isinstance(sb, dict) and not isinstance(sb, list) or len(sb) == 0:
        raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
    if isinstance(sb, dict):
        if any(not isinstance(ids, tuple) for ids in sb):
            raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
        if any(any((not _is_int(t) or t < 0) for t in ids) or len(ids) == 0 for ids in sb):
            raise ValueError("Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is "
                             f"{sb}.")
    else:
        def pair_ok(seq) -> bool:
            return (isinstance(seq[0], list) and all(_is_int(t) and t > 0 for t in seq[0])
                    and isinstance(seq[1], float))

        if any((not pair_ok(seq)) or len(seq) == 0 for seq in sb):
            raise ValueError("Each element in `sequence_bias` has to be a non-empty list of lists of positive "
                             f"integers and float, but is {sb}.")
    if isinstance(sb, dict) and any(not isinstance(b, float) for b in sb.values()):
        raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")


def validate_bad_words(bad_words_ids: Any) -> None:
    """NoBadWordsLogitsProcessor._validate_arguments."""
    bw = bad_words_ids
    if not isinstance(bw, list) or len(bw) == 0:
        raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
    if any(not isinstance(ids, list) for ids in bw):
        raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
    if any(any((not _is_int(t) or t < 0) for t in ids) for ids in bw):
        raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")


def _as_dict(sequence_bias: Any) -> Dict[Tuple[int, ...], float]:
    """_convert_list_arguments_into_dict: a repeated sequence keeps its first place and takes its last bias."""
    if isinstance(sequence_bias, dict):
        return dict(sequence_bias)
    return {tuple(ids): b for ids, b in sequence_bias}


def _check_vocab(d: Dict[Tuple[int, ...], float], vocab: Optional[int]) -> None:
    """_prepare_bias_variables' check (there at the first call, with the scores' width; here before any work)."""
    if vocab is None:
        return
    bad = [t for ids in d for t in ids if t >= vocab]
    if bad:
        raise ValueError(f"The model vocabulary size is {vocab}, but the following tokens were being biased: {bad}")


def _ordered(d: Dict[Tuple[int, ...], float]) -> List[Entry]:
    items = [(tuple(int(t) for t in ids), float(b)) for ids, b in d.items()]
    return [e for e in items if len(e[0]) == 1] + [e for e in items if len(e[0]) != 1]


def sequence_bias_entries(sequence_bias: Any, vocab: Optional[int] = None) -> List[Entry]:
    """The checked sequence_bias (dict {tuple: float} or list of [ids, float]) in table order."""
    validate_sequence_bias(sequence_bias)
    d = _as_dict(sequence_bias)
    _check_vocab(d, vocab)
    return _ordered(d)


def bad_words_entries(bad_words_ids: Any, eos: Optional[int] = None, vocab: Optional[int] = None) -> List[Entry]:
    """The checked bad_words_ids as -inf entries in table order; sequences equal to [eos] are dropped first, as
    NoBadWordsLogitsProcessor.__init__ does (nothing left: no entries, the processor then changes nothing). An empty
    sequence passes transformers' checks and fails in its first call with an IndexError; here it is a ValueError."""
    validate_bad_words(bad_words_ids)
    if any(len(ids) == 0 for ids in bad_words_ids):
        raise ValueError(f"Each list in `bad_words_ids` has to be non-empty, but is {bad_words_ids}.")
    kept = [ids for ids in bad_words_ids if eos is None or ids != [eos]]
    d = {tuple(ids): float("-inf") for ids in kept}
    _check_vocab(d, vocab)
    return _ordered(d)


def check_limits(pre: Sequence[Entry], post: Sequence[Entry]) -> None:
    """The kernel's table limits, as a ValueError before any work is queued."""
    if len(pre) + len(post) > MAX_ENTRIES:
        raise ValueError(f"sequence_bias + bad_words_ids: {len(pre)} + {len(post)} entries, this engine takes at most "
                         f"{MAX_ENTRIES}")
    longest = max((len(ids) for ids, _ in list(pre) + list(post)), default=0)
    if longest > MAX_IDS:
        raise ValueError(f"sequence_bias / bad_words_ids: an entry of {longest} ids, this engine takes at most "
                         f"{MAX_IDS} per entry")
