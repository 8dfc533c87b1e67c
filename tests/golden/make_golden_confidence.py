"""Golden vectors for per-token log-probabilities: transformers (5.15.0) on CPU in float32 with test-mini's seeded
synthetic weights on the FALLBACK_CLIPS features (task transcribe, max_new_tokens 40), written to confidence.json.

_retrieve_avg_logprobs is spied (generate() reaches it through _need_fallback once logprob_threshold is set; the
thresholds here are inert, one temperature 0.0, so nothing is re-decoded or skipped): per seek pass and row the
sequence it averaged over (EOS kept, pads cut) and the terms it sums, log_softmax(scores)[token] of generate()'s
processed scores.

Cases: greedy with timestamps, greedy without, greedy with repetition_penalty=1.3. Each case names its clips. The
penalised case replaces two of the FALLBACK_CLIPS: on "noise12" and "zeros30" the bf16 engine's penalised decode leaves
transformers' fp32 tokens at a near-tie (positions 11 and 19 of their first passes), so their positions could not be
compared one for one; "noise20" (white_noise(20.0, 3)) and "speech45" hold token equality on every pass.

Usage: python tests/golden/make_golden_confidence.py   (about a minute on 8 CPU cores)
"""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import make_golden as mg
from make_golden import DIMS, FALLBACK_CLIPS, SEED, clips
from make_golden_penalties import _model
from twamd.synth_audio import white_noise

INERT = {"temperature": (0.0,), "compression_ratio_threshold": 1e9, "logprob_threshold": -1e9}
RP_CLIPS = ("speech30", "noise20", "speech45")
CASES = [  # name, clips, generate kwargs
    ("greedy_ts", FALLBACK_CLIPS, {"return_timestamps": True}),
    ("greedy_no_ts", FALLBACK_CLIPS, {"return_timestamps": False}),
    ("greedy_ts_rp1.3", RP_CLIPS, {"return_timestamps": True, "repetition_penalty": 1.3}),
]


def _features(names):
    """The clips' first 30 s as the feature extractor hands them to generate() (one window each)."""
    from transformers import WhisperFeatureExtractor

    fe = WhisperFeatureExtractor(feature_size=DIMS.n_mels)
    cl = dict(clips(), noise20=white_noise(20.0, 3))
    return torch.from_numpy(np.stack([fe(cl[k], sampling_rate=16000, return_tensors="np")["input_features"][0]
                                      for k in names]))


def _spied(fn):
    """Run fn() with generate_with_fallback and _retrieve_avg_logprobs spied: the seek passes, each with its rows
    (chunk indices), seeks and, per row in order, the tokens and terms of the average."""
    from transformers.models.whisper import generation_whisper as gw

    cls = gw.WhisperGenerationMixin
    orig_fb, orig_lp = cls.generate_with_fallback, cls.__dict__["_retrieve_avg_logprobs"]
    passes, cur = [], []

    def lp_spy(scores, tokens, temperature):
        assert not temperature > 0.0
        sc = torch.stack(scores).to(tokens.device)
        tk = tokens
        if sc.shape[0] > tk.shape[0]:
            sc = sc[: tk.shape[0]]
        else:
            tk = tk[-sc.shape[0]:]
        lps = F.log_softmax(sc.float(), dim=-1)
        cur.append({"tokens": [int(t) for t in tk.tolist()],
                    "logprobs": [float(lps[i][tk[i]]) for i in range(lps.shape[0])]})
        return orig_lp.__func__(scores, tokens, temperature)

    def fb_spy(self, *a, **kw):
        del cur[:]
        r = orig_fb(self, *a, **kw)
        passes.append({"rows": [int(i) for i in kw["batch_idx_map"]], "seek": kw["seek"].tolist(),
                       "calls": list(cur)})
        return r

    cls.generate_with_fallback = fb_spy
    cls._retrieve_avg_logprobs = staticmethod(lp_spy)
    try:
        return fn(), passes
    finally:
        cls.generate_with_fallback = orig_fb
        cls._retrieve_avg_logprobs = orig_lp


def make(cases=CASES):
    res = []
    for name, names, kw in cases:
        feats = _features(names)
        m, _ = _model()
        with torch.no_grad():
            out, passes = _spied(lambda: m.generate(feats, task="transcribe", max_new_tokens=40, **INERT, **kw))
        for p in passes:  # one call per row of the pass, in row order (the only temperature never falls back)
            assert len(p["calls"]) == len(p["rows"]), name
        res.append({"name": name, "clips": list(names), "kwargs": kw, "sequences": out.tolist(), "passes": passes})
    return {"max_new_tokens": 40, "inert": {k: list(v) if isinstance(v, tuple) else v
                                                                          for k, v in INERT.items()}, "cases": res}


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(max(1, os.cpu_count() or 1))
    doc = {"seed": SEED, "dims": "test-mini", **make()}
    with open(os.path.join(mg.HERE, "confidence.json"), "w") as f:
        json.dump(doc, f)
    print("wrote confidence.json")
