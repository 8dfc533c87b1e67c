"""The three decode passes share one options record, one prompt phase and one pass scope (test-mini, 3 rows):
no pass leaves pass-scoped engine state behind, whatever it was called with and however it ended; the greedy
sample_pass decodes what decode_pass decodes from the same prompt; captured graphs are keyed by every option that
changes their launches, the log-probability flag included."""
import numpy as np
import pytest
import torch

from twamd import _lib
from twamd.engine import DecodeOptions
from twamd.pipeline import TurboTranscriber
from twamd.synth_audio import silence, speech_like, white_noise

pytestmark = pytest.mark.gpu
MAX_NEW = 12


def _engine(use_graphs=False):
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, max_beams=3, use_graphs=use_graphs)
    eng = t.engine
    host = np.zeros((3, 480000), np.float32)
    for i, c in enumerate([speech_like(30.0, 1234), white_noise(12.3, 7), silence(30.0)]):
        host[i, : len(c)] = c[:480000]
    eng.wave[:3].copy_(torch.from_numpy(host))
    eng.logmel(3)
    eng.row_map[:3] = torch.arange(3, dtype=torch.int32, device=eng.device)
    eng.seek[:3] = 0
    eng.encode(3)
    return eng


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def tail(eng):
    return eng.prompt_tail("transcribe", True)


@pytest.fixture(scope="module")
def fresh_plain(tail):
    """A plain greedy pass of an engine that has run nothing else."""
    with _engine() as e:
        return e.decode_pass(3, tail, None, MAX_NEW).tokens


def _prefix(eng):
    """Two tokens per row, the first a left pad: [pad, <|startofprev|>]."""
    return [[eng.gen.special.eot, eng.gen.suppress_tokens[-2]]] * 3, [1, 1, 1]


def _passes(eng, tail, **kw):
    ns = eng.gen.special.notimestamps - 1
    return {"decode": lambda: eng.decode_pass(3, tail, None, MAX_NEW, **kw),
            "sample": lambda: eng.sample_pass(3, tail, None, MAX_NEW, temperature=0.0, no_speech_token=ns, **kw),
            "beam": lambda: eng.beam_pass(3, 3, tail, None, MAX_NEW, criteria=True, no_speech_token=ns, **kw)}


def _assert_idle(eng):
    assert eng._masked is False and eng._align is None and eng._kv_tab is None
    assert eng._use_dec_row_map is False and eng._row_group == 1
    assert eng._opts == DecodeOptions() and not eng._opts.history and not eng._opts.token_logprobs


@pytest.mark.parametrize("which", ["decode", "sample", "beam"])
def test_a_pass_with_every_option_leaves_no_state(eng, tail, fresh_plain, which):
    res = _passes(eng, tail, prefix=_prefix(eng), align=True, token_logprobs=True, repetition_penalty=1.3)[which]()
    assert len(res.token_ts) == 3 and [len(lp) for lp in res.token_lp] == [len(t) for t in res.tokens]
    _assert_idle(eng)
    assert eng.decode_pass(3, tail, None, MAX_NEW).tokens == fresh_plain
    _assert_idle(eng)


def test_a_pass_that_raises_leaves_no_state(eng, tail, fresh_plain, monkeypatch):
    """4 windows x 3 beams are more rows than the engine has: a ValueError before any launch."""
    launched = []
    call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (launched.append(name), call(name, *a))[1])
    with pytest.raises(ValueError, match="decoder rows"):
        eng.beam_pass(4, 3, tail, None, MAX_NEW, prefix=([[1, 2]] * 4, [1] * 4), align=True, token_logprobs=True,
                      repetition_penalty=1.3)
    for name, run in _passes(eng, tail, top_p=0.9).items():  # an unknown option keyword: a TypeError, as ever
        with pytest.raises(TypeError, match="top_p"):
            run()
    assert launched == []
    _assert_idle(eng)
    assert eng.decode_pass(3, tail, None, MAX_NEW).tokens == fresh_plain


@pytest.mark.parametrize("case", ["detected", "given", "prefix"])
def test_greedy_sample_pass_decodes_what_decode_pass_decodes(eng, tail, case):
    """One prompt phase: languages detected at the SOT step, languages given per row, and a two-token prefix with a
    left pad in front of the init tokens."""
    lb = eng.gen.special.lang_begin
    langs = [lb + 1, lb + 2, lb] if case == "given" else None
    kw = {"prefix": _prefix(eng)} if case == "prefix" else {}
    a = eng.decode_pass(3, tail, langs, MAX_NEW, **kw)
    b = eng.sample_pass(3, tail, langs, MAX_NEW, temperature=0.0, **kw)
    assert a.tokens == b.tokens and a.lang_ids == b.lang_ids
    assert all(a.tokens) and (langs is None or a.lang_ids == langs)


def test_step_graphs_are_keyed_by_the_logprob_flag_and_the_penalty(tail):
    """One engine with captured graphs: with token_logprobs, plain, with a penalty, plain. Both plain passes equal a
    fresh engine's (a prompt or step graph that baked tw_token_logprob or the history pre-pass in would not)."""
    with _engine(use_graphs=True) as fresh:
        want = fresh.decode_pass(3, tail, None, MAX_NEW).tokens
    with _engine(use_graphs=True) as used:
        lp = used.decode_pass(3, tail, None, MAX_NEW, token_logprobs=True)
        assert lp.tokens == want and [len(x) for x in lp.token_lp] == [len(t) for t in want]
        assert used.decode_pass(3, tail, None, MAX_NEW).tokens == want
        pen = used.decode_pass(3, tail, None, MAX_NEW, repetition_penalty=1.5, no_repeat_ngram_size=1)
        assert pen.tokens != want
        plain = used.decode_pass(3, tail, None, MAX_NEW)
        assert plain.tokens == want and plain.token_lp is None
        n_graphs = len(used._graphs)
        assert used.decode_pass(3, tail, None, MAX_NEW, token_logprobs=True).token_lp == lp.token_lp
        assert len(used._graphs) == n_graphs  # (replayed, not captured again)
