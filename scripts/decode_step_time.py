"""Measurement (not a bench line): the greedy decode pass alone (no encoder beside it) at large-v3-turbo dims, per
decoder step (47 launches per token), for several row counts. One pass = the prompt graph (SOT, language
detection, task token) + 128 generated tokens with EOS suppressed, i.e. 130 decoder steps; the encoder runs once
before, untimed. Prints one JSON line per (rows, mode).

    python scripts/decode_step_time.py [--rows 15 24 64] [--reps 3] [--fused 0 1] [--penalties 0 1] [--beams 12 5]
                                       [--logprobs 0 1] [--alternatives 0 8] [--seqbias 0 1]

--fused 1: the decoder's layers as one persistent launch (tw_dec_fused) at every row count <= 32, 0: the launch chain
(WhisperEngine.dec_fused_alone / dec_fused_max_rows overridden); with both, each row count runs both and reports
whether their tokens agree.
--penalties 1: the passes run with repetition_penalty=1.3 and no_repeat_ngram_size=3 (tw_logits_history queued ahead
of every selection), 0: without; with both, the cost of the pre-pass is the difference of the two lines.
--seqbias 1: the passes run with a 64-entry table of 1 to 4 ids each, 32 sequence_bias entries and 32 bad_words_ids
(tw_logits_history_bias queued ahead of every selection; with --penalties 1 the same launch carries all four stages),
0: without; the cost is the difference of the two lines.
--logprobs 1: the passes run with token_logprobs (tw_token_logprob captured ahead of every selection; the beam pass
with run_tlp / fin_tlp), 0: without; with both, the cost of the pre-kernel is the difference of the two lines.
--alternatives K: the passes run with top_alternatives = K (tw_token_topk's two launches captured ahead of every
selection; the beam pass with one launch over all its rows and the fin_tab gather after it), 0: without; the cost is
the difference of the two lines.
--beams W NB: also the beam pass of W windows x NB beams (one captured step per token: decoder step over W * NB rows,
tw_beam_step), 128 tokens with EOS suppressed, per step from the pass's wall time.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "turbo-whisper-workspace_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from twamd.config import PRESETS, GenerationSettings  # noqa: E402
from twamd.engine import WhisperEngine  # noqa: E402
from twamd.synth_audio import workload  # noqa: E402
from twamd.weights import build_weights  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[15, 24, 64])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--check-every", type=int, nargs="+", default=[8])
    ap.add_argument("--graph-steps", type=int, nargs="+", default=[1])
    ap.add_argument("--fused", type=int, nargs="+", default=[0])
    ap.add_argument("--slope", type=int, default=0, help="also time 64-token passes: per-step slope without the "
                    "pass's fixed costs")
    ap.add_argument("--penalties", type=int, nargs="+", default=[0])
    ap.add_argument("--beams", type=int, nargs=2, default=None, metavar=("W", "NB"))
    ap.add_argument("--logprobs", type=int, nargs="+", default=[0])
    ap.add_argument("--alternatives", type=int, nargs="+", default=[0])
    ap.add_argument("--seqbias", type=int, nargs="+", default=[0])
    a = ap.parse_args()
    dims = PRESETS["large-v3-turbo"]
    gen = GenerationSettings.default(dims)
    B = max(a.rows + ([a.beams[0]] if a.beams else []))
    eng = WhisperEngine(build_weights(dims, seed=1234), gen, max_batch=B, device="cuda",
                        max_beams=a.beams[1] if a.beams else 1)
    eng.set_suppress_tokens(list(gen.suppress_tokens) + [gen.special.eot])
    eng.wave[:B].copy_(torch.from_numpy(workload(B, 30.0, seed=1234)))
    eng.logmel(B)
    tail = eng.prompt_tail("transcribe", True)
    # --seqbias: 64 entries of 1 to 4 text ids (seeded), the first 32 biased by +-2, the rest forbidden
    rng = np.random.default_rng(7)
    seqs = [[int(t) for t in rng.integers(1, gen.special.eot, 1 + e % 4)] for e in range(64)]
    table = {"sequence_bias": [[ids, 2.0 if e % 2 else -2.0] for e, ids in enumerate(seqs[:32])],
             "bad_words_ids": seqs[32:]}
    for R in a.rows:
        eng.row_map[:R] = torch.arange(R, dtype=torch.int32)
        eng.seek[:R] = 0
        eng.encode(R)
        torch.cuda.synchronize()
        ref = {}  # per (penalties, seqbias) value: the first mode's tokens
        for fz, ce, gs, pen, lpo, sbo, alt in [(f, c, g, p, q, b, k) for f in a.fused for c in a.check_every
                                               for g in a.graph_steps for p in a.penalties for q in a.logprobs
                                               for b in a.seqbias for k in a.alternatives]:
            if fz and R > 32:
                continue
            eng.dec_fused_alone = bool(fz)
            eng.dec_fused_max_rows = 32 if fz else 0
            eng.graph_steps_alone = gs
            eng._graphs.clear()
            hk = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3} if pen else {}
            if lpo:
                hk["token_logprobs"] = True
            if alt:
                hk["top_alternatives"] = alt
            if sbo:
                hk.update(table)
            eng.decode_pass(R, tail, None, 128, check_every=ce, **hk)  # warm-up: graph captures
            torch.cuda.synchronize()
            best = 1e9
            eng.pass_events = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                res = eng.decode_pass(R, tail, None, 128, check_every=ce, **hk)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            loop_us = min(e0.elapsed_time(e1) * 1e3 / n for e0, e1, n, _ in eng.pass_events)
            eng.pass_events = None
            print(json.dumps({"rows": R, "fused": fz, "check_every": ce, "graph_steps": gs, "penalties": pen,
                              "logprobs": lpo, "alternatives": alt, "seqbias": sbo,
                              "loop_us_per_step": round(loop_us, 1)}),
                  flush=True)
            assert all(len(t) == 128 for t in res.tokens)
            ref.setdefault((pen, sbo), res.tokens)
            if a.slope:
                eng.decode_pass(R, tail, None, 64, check_every=ce, **hk)
                torch.cuda.synchronize()
                b64 = 1e9
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    eng.decode_pass(R, tail, None, 64, check_every=ce, **hk)
                    torch.cuda.synchronize()
                    b64 = min(b64, time.perf_counter() - t0)
                print(json.dumps({"rows": R, "check_every": ce, "graph_steps": gs, "penalties": pen,
                                  "pass64_ms": round(b64 * 1e3, 2),
                                  "slope_us_per_step": round((best - b64) * 1e6 / 64, 1),
                                  "fixed_ms": round((b64 - 66 * (best - b64) / 64) * 1e3, 2)}), flush=True)
            print(json.dumps({"rows": R, "fused": fz, "check_every": ce, "graph_steps": gs, "penalties": pen,
                              "logprobs": lpo, "alternatives": alt, "seqbias": sbo, "pass_ms": round(best * 1e3, 2),
                              "step_us": round(best * 1e6 / 130, 1), "tokens_equal": res.tokens == ref[(pen, sbo)]}),
                  flush=True)
    if a.beams:
        W, nb = a.beams
        eng.row_map[:W] = torch.arange(W, dtype=torch.int32)
        eng.seek[:W] = 0
        eng.encode(W)
        torch.cuda.synchronize()
        for pen, lpo, alt in [(p, q, k) for p in a.penalties for q in a.logprobs for k in a.alternatives]:
            hk = {"repetition_penalty": 1.3, "no_repeat_ngram_size": 3} if pen else {}
            if lpo:
                hk["token_logprobs"] = True
            if alt:
                hk["top_alternatives"] = alt
            eng.beam_pass(W, nb, tail, None, 128, **hk)  # warm-up: graph capture
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(a.reps):
                t0 = time.perf_counter()
                eng.beam_pass(W, nb, tail, None, 128, **hk)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            print(json.dumps({"beam_windows": W, "num_beams": nb, "rows": W * nb, "penalties": pen, "logprobs": lpo,
                              "alternatives": alt, "pass_ms": round(best * 1e3, 2), "step_us": round(best * 1e6 / 130, 1)}), flush=True)


if __name__ == "__main__":
    main()
