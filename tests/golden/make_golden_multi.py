"""Golden vectors for the list call: transformers' (5.15.0) own ASR pipeline on CPU in float32 with test-mini's
seeded synthetic weights, called with a LIST of inputs, written to multi.json.

Every case stores the list call's results ("list_output"), the results of the same call on every input alone
("single_outputs"), whether the two agree ("list_differs_from_singles"), and, per input, the model outputs the list
call's postprocess() received for its windows ("windows": tokens, stride, token_timestamps), so that decode_asr can
be checked input by input without a model.

Inputs (INPUTS): "mix75" = speech_like(40, 5) + white_noise(35, 11) (75 s), "noise12" = white_noise(12.3, 7),
"speech45" = speech_like(45, 99), "mix20" = the first 20 s of mix75, "zeros30" = 30 s of silence.

The word case looks for inputs at which the DataLoader's batches (consecutive windows ACROSS input boundaries)
give other word times than per-input batches: WORD_SETS are tried in order (at most three) and the first whose
list result differs from its single results is kept; the flag says whether one was found.

Usage: python tests/golden/make_golden_multi.py   (a few minutes on 8 CPU cores)
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch

import make_golden as mg
from make_golden import ALIGN_HEADS_MINI, DIMS, SEED, _jsonable, clips, hf_model, hf_tokenizer
from oracle import whisper_oracle as wo
from twamd.config import GenerationSettings
from twamd.synth_audio import speech_like, white_noise

MAX_NEW = 24
CASES = [  # name, inputs, pipeline kwargs, extra generate kwargs, return_timestamps
    ("chunk_30_5_b4", ("mix75", "noise12", "speech45"), dict(chunk_length_s=30, stride_length_s=5, batch_size=4), {},
     True),
    ("ref_60_5_b32", ("mix75", "noise12", "speech45"), dict(chunk_length_s=60, stride_length_s=5, batch_size=32), {},
     True),
    ("nochunk_short_b2", ("noise12", "mix20"), dict(batch_size=2), {}, True),
    ("nochunk_mixed_b1", ("mix75", "noise12"), dict(batch_size=1), {}, True),
    ("beam3_30_5_b4", ("mix75", "noise12", "speech45"), dict(chunk_length_s=30, stride_length_s=5, batch_size=4),
     {"num_beams": 3}, True),
]
WORD_KW = dict(chunk_length_s=30, stride_length_s=5, batch_size=2)
WORD_SETS = [("mix75", "zeros30", "speech45"), ("zeros30", "noise12", "speech45"), ("noise12", "zeros30", "mix75")]


def inputs():
    mix = np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)])
    cl = clips()
    return {"mix75": mix, "noise12": cl["noise12"], "speech45": cl["speech45"], "mix20": mix[: 20 * 16000],
            "zeros30": cl["zeros30"]}


def _pipe(word=False):
    from transformers import AutomaticSpeechRecognitionPipeline, WhisperFeatureExtractor

    gen = GenerationSettings.default(DIMS)
    sd = wo.synth_state_dict(DIMS.d_model, DIMS.encoder_layers, DIMS.decoder_layers, DIMS.ffn, DIMS.n_mels,
                             DIMS.vocab, SEED)
    m = hf_model(DIMS, sd, gen)
    if word:
        m.generation_config.alignment_heads = ALIGN_HEADS_MINI
    return AutomaticSpeechRecognitionPipeline(model=m, feature_extractor=WhisperFeatureExtractor(
        feature_size=DIMS.n_mels), tokenizer=hf_tokenizer(gen.special), device=-1)


def _run(pipe, names, kw, gk, rt):
    """(list result, single results, per input the model outputs of the list call's windows)."""
    x = inputs()
    call = dict(generate_kwargs={"task": "transcribe", "num_beams": 1, "max_new_tokens": MAX_NEW, **gk},
                return_timestamps=rt, **kw)
    seen = []
    orig = pipe.postprocess

    def spy(model_outputs, *a, **k):
        seen.append([{"tokens": o["tokens"][0].tolist(),
                      # (samples here; postprocess() turns them into seconds with this division)
                      **({"stride": [s / 16000 for s in o["stride"]]} if o.get("stride") is not None else {}),
                      **({"token_timestamps": [float(np.float32(t)) for t in o["token_timestamps"][0].tolist()]}
                         if o.get("token_timestamps") is not None else {})} for o in model_outputs])
        return orig(model_outputs, *a, **k)

    pipe.postprocess = spy
    try:
        listed = pipe([x[n].copy() for n in names], **call)
    finally:
        pipe.postprocess = orig
    singles = [pipe(x[n].copy(), **call) for n in names]
    assert isinstance(listed, list) and len(listed) == len(names) == len(seen)
    return _jsonable(listed), _jsonable(singles), seen


def make():
    cases = []
    pipe = _pipe()
    for name, names, kw, gk, rt in CASES:
        listed, singles, seen = _run(pipe, names, kw, gk, rt)
        cases.append({"name": name, "inputs": list(names), "kwargs": kw, "generate_kwargs": gk,
                      "return_timestamps": rt, "list_output": listed, "single_outputs": singles, "windows": seen,
                      "list_differs_from_singles": listed != singles})
        print(name, "differs" if listed != singles else "equal")
    pipe = _pipe(word=True)
    for names in WORD_SETS:
        listed, singles, seen = _run(pipe, names, WORD_KW, {}, "word")
        print("word_30_5_b2", names, "differs" if listed != singles else "equal")
        if listed != singles:
            break
    cases.append({"name": "word_30_5_b2", "inputs": list(names), "kwargs": WORD_KW, "generate_kwargs": {},
                  "return_timestamps": "word", "list_output": listed, "single_outputs": singles, "windows": seen,
                  "list_differs_from_singles": listed != singles})
    return cases


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    doc = {"seed": SEED, "dims": "test-mini", "max_new_tokens": MAX_NEW, "alignment_heads": ALIGN_HEADS_MINI,
           "cases": make()}
    with open(os.path.join(mg.HERE, "multi.json"), "w") as f:
        json.dump(doc, f)
    print("wrote multi.json")
