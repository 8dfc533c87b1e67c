"""Forced alignment timings on large-v3-turbo with synthetic weights: 24 windows, 100 forced tokens each.

Reports, as one JSON line (also written to --out):
  post_host_ms / post_gpu_ms   the alignment post-processing on the same recorded probabilities, median of --runs
                               runs after --warmup: host = device-to-host copy of the probabilities + alignment.
                               token_timestamps per row (what _token_ts does); gpu = tw_align_cost + the copy of the
                               cropped costs + tw_dtw per row (WhisperEngine._force_times)
  force_step_us / hook_step_us the decode steps of force_pass (captured step + tw_logits_force, no host sync) against
                               the same tokens driven through decode_pass with a step_hook (a host round trip per
                               token), device events around the steps, per step
  align_cost_us / _tbps        tw_align_cost alone (device events, median) and its achieved bytes/s: two reads of the
                               probabilities it uses plus one write of the costs, over the kernel time

usage: python scripts/align_time.py [--rows 24] [--tokens 100] [--runs 20] [--warmup 5] [--out profiles/align_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "turbo-whisper-workspace_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from twamd import _lib, alignment  # noqa: E402
from twamd.engine import S_ENC  # noqa: E402
from twamd.pipeline import TurboTranscriber  # noqa: E402
from twamd.synth_audio import workload  # noqa: E402

TURBO_HEADS = [(2, 4), (2, 11), (3, 3), (3, 6), (3, 11), (3, 14)]  # openai/whisper-large-v3-turbo's alignment heads


def median_ms(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=24)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "align_time.py measures on the GPU"
    R, L = a.rows, a.tokens
    tr = TurboTranscriber.from_pretrained("large-v3-turbo", seed=1234, max_batch=R, max_beams=1)
    eng = tr.engine
    eng.gen.alignment_heads = list(TURBO_HEADS)
    st = eng.gen.special
    rng = np.random.default_rng(7)
    forced = [[int(t) for t in rng.integers(300, 40000, L)] for _ in range(R)]
    nf = [3000] * R
    eng.wave[:R].copy_(torch.from_numpy(workload(R, 30.0, seed=1234)))
    eng.logmel(R)
    eng.encode(R, row_map=False, seek=False)
    tail = eng.prompt_tail("transcribe", False)
    P = eng._prompt_len(tail)

    # ---- forced decode: force_pass's steps against decode_pass + step_hook on the same tokens
    eng.pass_events = []
    for _ in range(3):
        res = eng.force_pass(R, tail, None, forced, num_frames=nf)
    torch.cuda.synchronize()
    ev = eng.pass_events[1:]
    force_us = statistics.median(e0.elapsed_time(e1) * 1e3 / n for e0, e1, n, _ in ev)
    force_host_us = statistics.median(h * 1e6 / n for _, _, n, h in ev)
    table = torch.tensor(forced, dtype=torch.int32, device=eng.device)

    def hook(k, v):
        if k < L:
            eng.ids[:R] = table[:, k]
            if v is not None:
                eng.embed_head(v)

    eng.set_suppress_tokens(list(eng.gen.suppress_tokens) + [st.eot])  # (no row finishes before the last token)
    eng.pass_events, eng.step_hook = [], hook
    try:
        for _ in range(3):
            eng.decode_pass(R, tail, None, L + 1, use_timestamps=False, align=True, num_frames=nf)  # (same kernels)
    finally:
        eng.step_hook = None
        eng.set_suppress_tokens(list(eng.gen.suppress_tokens))
    torch.cuda.synchronize()
    ev = eng.pass_events[1:]
    eng.pass_events = None
    hook_us = statistics.median(e0.elapsed_time(e1) * 1e3 / n for e0, e1, n, _ in ev)
    hook_host_us = statistics.median(h * 1e6 / n for _, _, n, h in ev)

    # ---- post-processing, both versions on the probabilities the last force_pass recorded
    eng.force_pass(R, tail, None, forced, num_frames=nf)
    eng._align_setup(R, P, L + 1)  # (the recording buffer of that pass, as _force_times / _token_ts read it)
    al = eng._align
    n_rows = [L] * R
    probs = al["buf"][: R * (L + 1) * al["n_slots"] * S_ENC].view(R, L + 1, al["n_slots"], S_ENC)
    out = {}

    def post_host():
        w = probs[:, :L].permute(0, 2, 1, 3)[:, al["perm"]].float().cpu().numpy()
        out["host"] = [alignment.token_timestamps(w[r], 0, nf[r], eng.gen.median_filter_width) for r in range(R)]

    def post_gpu():
        with torch.cuda.stream(eng.stream):
            out["gpu"] = eng._force_times(R, n_rows, nf)

    def kernel():
        _lib.call("tw_align_cost", al["buf"].data_ptr(), R, L + 1, al["n_slots"], S_ENC,
                  eng._force_ext[0].data_ptr(), eng._force_ext[1].data_ptr(), eng.gen.median_filter_width,
                  eng._force_cost.data_ptr(), torch.cuda.current_stream().cuda_stream)

    try:
        gpu_ms = median_ms(post_gpu, a.warmup, a.runs)
        host_ms = median_ms(post_host, a.warmup, a.runs)
        for _ in range(a.warmup):
            kernel()
        ks = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            kernel()
            e1.record()
            torch.cuda.synchronize()
            ks.append(e0.elapsed_time(e1) * 1e3)
    finally:
        eng._align = None
    k_us = statistics.median(ks)
    nbytes = R * L * S_ENC * 4 * (2 * al["n_slots"] + 1)
    same = float(np.mean([np.mean(np.abs(g - h) < 1e-6) for g, h in zip(out["gpu"], out["host"])]))
    rec = {"model": "large-v3-turbo (synthetic)", "rows": R, "tokens": L, "slots": al["n_slots"],
           "runs": a.runs, "warmup": a.warmup,
           "post_host_ms": round(host_ms[0], 2), "post_host_ms_min_max": [round(host_ms[1], 2), round(host_ms[2], 2)],
           "post_gpu_ms": round(gpu_ms[0], 2), "post_gpu_ms_min_max": [round(gpu_ms[1], 2), round(gpu_ms[2], 2)],
           "times_equal_frac_gpu_vs_host": round(same, 4),
           "force_step_us": round(force_us, 1), "force_host_us_per_step": round(force_host_us, 1),
           "hook_step_us": round(hook_us, 1), "hook_host_us_per_step": round(hook_host_us, 1),
           "align_cost_us": round(k_us, 1), "align_cost_bytes": nbytes,
           "align_cost_tbps": round(nbytes / (k_us * 1e-6) / 1e12, 3),
           "probs_mb": round(R * L * al["n_slots"] * S_ENC * 4 / 1e6, 1),
           "lp_mean": round(float(np.mean([np.mean(x) for x in res.token_lp])), 3)}
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
