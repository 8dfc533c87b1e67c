"""Golden vectors for repetition_penalty / no_repeat_ngram_size / length_penalty: transformers (5.15.0) on CPU in float32
with test-mini's seeded synthetic weights, written to penalties.json. Every case records its twin without the option,
so a test can tell that the option changed something.

  "generate"   WhisperForConditionalGeneration.generate() on the FALLBACK_CLIPS features (task transcribe): greedy and
               beam cases, with every seek pass's decoder prompt and raw output (spied from generate_with_fallback)
  "fallback"   the fallback criteria under repetition_penalty=1.3 (inert thresholds, the spied _need_fallback, as
               make_golden.make_fallback's "metrics" case): the average log-probability of the penalised scores
  "pipeline"   the ASR pipeline on the options.json audio: the reference call with repetition_penalty=1.3 and
               no_repeat_ngram_size=3, greedy and as shipped (beam 5), and one unchunked long-form call with
               condition_on_prev_tokens and no_repeat_ngram_size=3

Usage: python tests/golden/make_golden_penalties.py   (a few minutes on 8 CPU cores)
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

import make_golden as mg
from make_golden import DIMS, FALLBACK_CLIPS, SEED, GenerationSettings, _jsonable, clips, hf_model, hf_tokenizer, wo
from twamd.synth_audio import speech_like, white_noise

PROMPT = mg.PROMPT_TOKENS[:3]  # the short prompt's text tokens (prompt_ids = [<|startofprev|>] + these)
GENERATE_CASES = [  # name, generate kwargs of the case, kwargs shared with its twin
    ("greedy_rp", {"repetition_penalty": 1.3}, {"return_timestamps": True, "max_new_tokens": 40}),
    ("greedy_ngram2", {"no_repeat_ngram_size": 2}, {"return_timestamps": True, "max_new_tokens": 40}),
    ("greedy_rp_ngram3", {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3},
     {"return_timestamps": True, "max_new_tokens": 40}),
    ("greedy_rp_ngram3_no_ts", {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3},
     {"return_timestamps": False, "max_new_tokens": 40}),
    ("greedy_prompt_rp_ngram2", {"repetition_penalty": 1.3, "no_repeat_ngram_size": 2},
     {"return_timestamps": True, "max_new_tokens": 40, "prompt": True}),
    ("beam3_rp_ngram2", {"repetition_penalty": 1.3, "no_repeat_ngram_size": 2},
     {"return_timestamps": True, "max_new_tokens": 24, "num_beams": 3}),
    ("beam3_lp0.5", {"length_penalty": 0.5}, {"return_timestamps": True, "max_new_tokens": 40, "num_beams": 3}),
    ("beam3_lp2.0", {"length_penalty": 2.0}, {"return_timestamps": True, "max_new_tokens": 40, "num_beams": 3}),
]


def _model():
    d = DIMS
    gen = GenerationSettings.default(d)
    sd = wo.synth_state_dict(d.d_model, d.encoder_layers, d.decoder_layers, d.ffn, d.n_mels, d.vocab, SEED)
    m = hf_model(d, sd, gen)
    # <|startofprev|> as make_golden.make_prompt names it (suppress_tokens[-2])
    m.generation_config.prev_sot_token_id = int(m.generation_config.suppress_tokens[-2])
    return m, gen


def _spied(fn):
    """Run fn() with generate_with_fallback spied: returns (fn's result, the seek passes' prompts and raw outputs)."""
    from transformers.models.whisper import generation_whisper as gw

    orig = gw.WhisperGenerationMixin.generate_with_fallback
    log = []

    def spy(self, *a, **kw):
        r = orig(self, *a, **kw)
        log.append({"prompts": kw["decoder_input_ids"].tolist(), "rows": [int(i) for i in kw["batch_idx_map"]],
                    "seek": kw["seek"].tolist(), "sequences": [x.tolist() for x in r[0]]})
        return r

    gw.WhisperGenerationMixin.generate_with_fallback = spy
    try:
        return fn(), log
    finally:
        gw.WhisperGenerationMixin.generate_with_fallback = orig


def _features():
    from transformers import WhisperFeatureExtractor

    fe = WhisperFeatureExtractor(feature_size=DIMS.n_mels)
    cl = clips()
    return torch.from_numpy(np.stack([fe(cl[k], sampling_rate=16000, return_tensors="np")["input_features"][0]
                                      for k in FALLBACK_CLIPS]))


def make_generate():
    feats = _features()
    m, _ = _model()
    prompt_ids = [int(m.generation_config.prev_sot_token_id)] + PROMPT
    res, twins = [], {}
    for name, opts, shared in GENERATE_CASES:
        kw = {k: v for k, v in shared.items() if k != "prompt"}
        if shared.get("prompt"):
            kw["prompt_ids"] = torch.tensor(prompt_ids)

        def run(extra):
            with torch.no_grad():
                o, log = _spied(lambda: m.generate(feats, task="transcribe", **kw, **extra))
            return {"sequences": o.tolist(), "passes": log}

        key = json.dumps(shared, sort_keys=True)
        if key not in twins:  # the same call without the option
            twins[key] = run({})
        got = run(opts)
        differs = got["sequences"] != twins[key]["sequences"]
        # (no length_penalty from -4 to 8 changes generate()'s output on these clips, at 24 or 40 new tokens, nor the
        # pipeline's on the 75-s audio: the two cases pin exactness; tests/test_gpu_history.py and
        # test_gpu_penalties.py::test_length_penalty_reaches_the_beam_kernel show the exponent acting and arriving)
        assert differs or "length_penalty" in opts, name
        res.append({"name": name, "options": opts, "shared": shared, **got, "differs_from_plain": differs,
                    "plain": twins[key]})
    return {"clips": list(FALLBACK_CLIPS), "prompt_ids": prompt_ids, "cases": res}


def make_fallback():
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    from transformers.models.whisper.generation_whisper import _get_attr_from_logit_processors

    feats = _features()
    kw = {"temperature": [0.0], "compression_ratio_threshold": 1e9, "logprob_threshold": -1e9,
          "no_speech_threshold": 2.0}
    out = {"kwargs": kw, "max_new_tokens": 40, "repetition_penalty": 1.3}
    for name, extra in (("calls", {"repetition_penalty": 1.3}), ("plain_calls", {})):
        m, _ = _model()
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
    return out


def make_pipeline():
    from transformers import AutomaticSpeechRecognitionPipeline, WhisperFeatureExtractor

    m, gen = _model()
    fe = WhisperFeatureExtractor(feature_size=DIMS.n_mels)
    pipe = AutomaticSpeechRecognitionPipeline(model=m, feature_extractor=fe, tokenizer=hf_tokenizer(gen.special),
                                              device=-1)
    audio = np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)]).astype(np.float32)
    ref = dict(chunk_length_s=60, stride_length_s=5, batch_size=32)
    both = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3}
    cases = [
        ("ref_call_greedy", ref, {"task": "transcribe", "num_beams": 1, "max_new_tokens": 24}, both),
        ("ref_call_as_shipped", ref, {"task": "transcribe", "max_new_tokens": 24}, both),
        ("long_cond_ngram3", {}, {"task": "transcribe", "num_beams": 1, "max_new_tokens": 40,
                                  "condition_on_prev_tokens": True}, {"no_repeat_ngram_size": 3}),
    ]
    res = []
    for name, kw, gk, opts in cases:
        out, log = _spied(lambda: pipe(audio.copy(), generate_kwargs=dict(gk, **opts), return_timestamps=True, **kw))
        plain, plog = _spied(lambda: pipe(audio.copy(), generate_kwargs=dict(gk), return_timestamps=True, **kw))
        assert out != plain, name
        res.append({"name": name, "kwargs": kw, "generate_kwargs": gk, "options": opts, "return_timestamps": True,
                    "output": _jsonable(out), "passes": log, "plain": {"output": _jsonable(plain), "passes": plog}})
    return {"audio": "speech_like(40,5)+white_noise(35,11)", "cases": res}


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    doc = {"seed": SEED, "dims": "test-mini", "generate": make_generate(), "fallback": make_fallback(),
           "pipeline": make_pipeline()}
    with open(os.path.join(mg.HERE, "penalties.json"), "w") as f:
        json.dump(doc, f)
    print("wrote penalties.json")
