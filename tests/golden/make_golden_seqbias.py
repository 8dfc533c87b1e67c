"""Golden vectors for sequence_bias / bad_words_ids: transformers (5.15.0) on CPU in float32 with test-mini's seeded
synthetic weights, written to seqbias.json. Every case records its twin without the options and the script asserts
that the two differ; the biased and forbidden ids are taken from the twin's own output so that each case fires.

  "generate"   WhisperForConditionalGeneration.generate() on the FALLBACK_CLIPS features (task transcribe): greedy and
               beam cases, with every seek pass's decoder prompt and raw output (spied from generate_with_fallback)
  "fallback"   the fallback criteria under sequence_bias (inert thresholds, the spied _need_fallback, as
               make_golden_penalties.make_fallback): the average log-probability of the biased scores
  "pipeline"   the ASR pipeline on the options.json audio: the reference call with both options (greedy), and one
               unchunked long-form call with condition_on_prev_tokens and bad_words_ids (the engine's callable refuses
               bad_words_ids: the tests hand it these sequences as -inf sequence_bias entries, and the kwargs as
               recorded here to transcribe_windows / WhisperEngine.generate)

Usage: python tests/golden/make_golden_seqbias.py   (a few minutes on 8 CPU cores)
"""
from __future__ import annotations

import json
import os
from collections import Counter

import numpy as np
import torch

import make_golden as mg
import make_golden_penalties as mp
from make_golden import _jsonable, hf_tokenizer
from twamd.synth_audio import speech_like, white_noise

EOT = 50257
BOOST = 9  # a text id no plain output holds: a positive 1-token bias on it rewrites the greedy outputs


def _options(rows, ban_first=False):
    """sequence_bias and bad_words_ids from the plain outputs (one list of generated ids per row): 1- and 2-token
    entries, positive and negative, several ending in the same id; bad words with a 2-token and a 1-token sequence.
    (a, b) is the first pair of adjacent text tokens, so the 2-token entries fire. ban_first: also the first row's
    first text token (long-form: only what lies before a pass's last timestamp pair reaches the output)."""
    a, b = next((int(r[i]), int(r[i + 1])) for r in rows for i in range(len(r) - 1) if r[i] < EOT and r[i + 1] < EOT)
    others = [int(t) for r in rows for t in r if t < EOT and t not in (a, b)]
    common = Counter(others).most_common(2)
    x = common[0][0]
    y = common[1][0] if len(common) > 1 else x
    # ([a, BOOST] and [b, BOOST] are one key when a == b: the later bias then replaces the earlier, as in transformers)
    sb = [[[BOOST], 6.0], [[a, b], -30.0], [[x], -4.0], [[a, BOOST], 3.5], [[b, BOOST], -1.25],
          [[BOOST, BOOST], -2.0], [[BOOST, a], 2.5]]
    bw = [[a, b], [y]]
    if ban_first:
        bw.append([next(int(t) for t in rows[0] if t < EOT)])
    return sb, bw


def _plain_rows(passes):
    return [[int(t) for t in s] for pl in passes for s in pl["sequences"]]  # (generated tokens, prompt cut off)


def make_generate():
    feats = mp._features()
    m, _ = mp._model()
    prompt_ids = [int(m.generation_config.prev_sot_token_id)] + mp.PROMPT
    both = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 2}
    cases = [  # name, which options, other generate kwargs of the case, kwargs shared with its twin
        ("greedy_sb", ("sb",), {}, {"return_timestamps": True, "max_new_tokens": 40}),
        ("greedy_bw", ("bw",), {}, {"return_timestamps": True, "max_new_tokens": 40}),
        ("greedy_sb_bw_rp_ngram2", ("sb", "bw"), both, {"return_timestamps": True, "max_new_tokens": 40}),
        ("greedy_prompt_sb_bw_rp_ngram2", ("sb", "bw"), both,
         {"return_timestamps": True, "max_new_tokens": 40, "prompt": True}),
        ("beam3_sb_bw", ("sb", "bw"), {}, {"return_timestamps": True, "max_new_tokens": 24, "num_beams": 3}),
    ]
    res, twins = [], {}
    for name, which, extra, shared in cases:
        kw = {k: v for k, v in shared.items() if k != "prompt"}
        if shared.get("prompt"):
            kw["prompt_ids"] = torch.tensor(prompt_ids)

        def run(opts):
            with torch.no_grad():
                o, log = mp._spied(lambda: m.generate(feats, task="transcribe", **kw, **opts))
            return {"sequences": o.tolist(), "passes": log}

        key = json.dumps(shared, sort_keys=True)
        if key not in twins:  # the same call with no option at all
            twins[key] = run({})
        sb, bw = _options(_plain_rows(twins[key]["passes"][:1]))
        opts = dict(extra)
        if "sb" in which:
            opts["sequence_bias"] = sb
        if "bw" in which:
            opts["bad_words_ids"] = bw
        got = run(json.loads(json.dumps(opts)))
        assert got["sequences"] != twins[key]["sequences"], name
        if extra:  # the options also act on top of the penalties (the order of the stages matters there)
            assert got["sequences"] != run(dict(extra))["sequences"], name
        res.append({"name": name, "options": opts, "shared": shared, **got, "plain": twins[key]})
    return {"clips": list(mg.FALLBACK_CLIPS), "prompt_ids": prompt_ids, "cases": res}


def make_fallback(sb):
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    from transformers.models.whisper.generation_whisper import _get_attr_from_logit_processors

    feats = mp._features()
    kw = {"temperature": [0.0], "compression_ratio_threshold": 1e9, "logprob_threshold": -1e9,
          "no_speech_threshold": 2.0}
    out = {"kwargs": kw, "max_new_tokens": 40, "sequence_bias": sb}
    for name, extra in (("calls", {"sequence_bias": json.loads(json.dumps(sb))}), ("plain_calls", {})):
        m, _ = mp._model()
        rec = []
        orig = m._need_fallback

        def spy(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature,
                _m=m, _orig=orig, _rec=rec):
            cr = _m._retrieve_compression_ratio(seek_sequence, vocab_size)
            lp = _m._retrieve_avg_logprobs(seek_outputs[index]["scores"], seek_sequence, temperature)
            nsp = _get_attr_from_logit_processors(logits_processor, WhisperNoSpeechDetection, "no_speech_prob")
            o = _orig(seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature)
            _rec.append({"index": int(index), "tokens": [int(t) for t in seek_sequence.tolist()],
                         "compression_ratio": float(cr), "avg_logprob": float(lp),
                         "no_speech_prob": None if nsp is None else float(nsp[index]),
                         "needs_fallback": bool(o[0]), "should_skip": bool(o[1])})
            return o

        m._need_fallback = spy
        with torch.no_grad():
            m.generate(feats, task="transcribe", return_timestamps=True, max_new_tokens=40, return_segments=True,
                       temperature=tuple(kw["temperature"]), **{k: v for k, v in kw.items() if k != "temperature"},
                       **extra)
        out[name] = rec
    assert [c["tokens"] for c in out["calls"]] != [c["tokens"] for c in out["plain_calls"]]
    return out


def make_pipeline():
    from transformers import AutomaticSpeechRecognitionPipeline, WhisperFeatureExtractor

    m, gen = mp._model()
    fe = WhisperFeatureExtractor(feature_size=mg.DIMS.n_mels)
    pipe = AutomaticSpeechRecognitionPipeline(model=m, feature_extractor=fe, tokenizer=hf_tokenizer(gen.special),
                                              device=-1)
    audio = np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)]).astype(np.float32)
    ref = dict(chunk_length_s=60, stride_length_s=5, batch_size=32)
    cases = [
        ("ref_call_greedy_sb_bw", ref, {"task": "transcribe", "num_beams": 1, "max_new_tokens": 24}, ("sb", "bw")),
        ("long_cond_bw", {}, {"task": "transcribe", "num_beams": 1, "max_new_tokens": 40,
                              "condition_on_prev_tokens": True}, ("bw",)),
    ]
    res = []
    for name, kw, gk, which in cases:
        plain, plog = mp._spied(lambda: pipe(audio.copy(), generate_kwargs=dict(gk), return_timestamps=True, **kw))
        sb, bw = _options(_plain_rows(plog), ban_first=not kw)
        opts = {}
        if "sb" in which:
            opts["sequence_bias"] = sb
        if "bw" in which:
            opts["bad_words_ids"] = bw
        out, log = mp._spied(lambda: pipe(audio.copy(), generate_kwargs=dict(gk, **json.loads(json.dumps(opts))),
                                          return_timestamps=True, **kw))
        assert out != plain and log != plog, name
        res.append({"name": name, "kwargs": kw, "generate_kwargs": gk, "options": opts, "return_timestamps": True,
                    "output": _jsonable(out), "passes": log, "plain": {"output": _jsonable(plain), "passes": plog}})
    return {"audio": "speech_like(40,5)+white_noise(35,11)", "cases": res}


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    gen = make_generate()
    doc = {"seed": mg.SEED, "dims": "test-mini", "generate": gen,
           "fallback": make_fallback(gen["cases"][0]["options"]["sequence_bias"]), "pipeline": make_pipeline()}
    with open(os.path.join(mg.HERE, "seqbias.json"), "w") as f:
        json.dump(doc, f)
    print("wrote seqbias.json")
