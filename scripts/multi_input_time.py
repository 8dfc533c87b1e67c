"""Measurement (not a bench line): what the list call buys over a loop of single calls, and what the gather kernel
costs beside the slice launches it replaced. Writes profiles/multi_input_time.json.

large-v3-turbo with synthetic weights on one GPU, greedy, chunk_length_s=30, stride_length_s=0, timestamps,
max_new_tokens=64. Medians of --runs runs after --warmup warm-ups.

  * list call vs loop: N clips of 20 s (synth_audio.workload) in ONE call, and the same clips in N single calls on
    the same engine (the only form the callable had before the list call: the baseline). Host clock around work
    that ends in a device synchronise. RTF = audio seconds / wall seconds.
  * tw_gather_windows at 24 x 480000 out of a 24-window arena with device events (a run of --reps launches between
    two events), beside the 2 x 24 slice launches (copy_ + zero_ per window) it replaced; 30-s windows (no zero
    tail) and 20-s windows. Achieved bytes/s = (bytes read from the arena + bytes written to the rows) / time.

    python scripts/multi_input_time.py [--clips 24 96] [--runs 20] [--warmup 5] [--out profiles/multi_input_time.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "turbo-whisper-workspace_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from twamd import _lib  # noqa: E402
from twamd.pipeline import TurboTranscriber  # noqa: E402
from twamd.synth_audio import workload  # noqa: E402

CHUNK = 480000
COPY_RATE_TBS = 6.3  # the HBM copy rate DESIGN quotes


def wall(fn, runs, warmup):
    """Median wall seconds of fn() (each run ends in a device synchronise), and the runs."""
    ts = []
    for k in range(warmup + runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def device_us(fn, reps, runs, warmup):
    """Median microseconds per fn() from device events around `reps` back-to-back calls."""
    out = []
    for k in range(warmup + runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(out)


def list_vs_loop(tr, n, a):
    clips = [np.ascontiguousarray(r) for r in workload(n, 20.0, seed=1234)]
    kw = dict(chunk_length_s=30, stride_length_s=0, batch_size=tr.engine.max_batch, return_timestamps=True,
              generate_kwargs={"task": "transcribe", "num_beams": 1, "max_new_tokens": 64})
    listed = tr(clips, **kw)
    equal = listed == [tr(c, **kw) for c in clips]
    t_list, _ = wall(lambda: tr(clips, **kw), a.runs, a.warmup)
    t_loop, _ = wall(lambda: [tr(c, **kw) for c in clips], a.runs, a.warmup)
    secs = 20.0 * n
    return {"clips": n, "clip_seconds": 20.0, "list_call_s": t_list, "loop_s": t_loop, "rtf_list": secs / t_list,
            "rtf_loop": secs / t_loop, "loop_over_list": t_loop / t_list, "results_equal": bool(equal)}


def gather_vs_slices(tr, seconds, a):
    eng = tr.engine
    rows, n = 24, int(seconds * 16000)
    arena = torch.randn(rows * n, device=eng.device)
    start = (ctypes.c_int64 * rows)(*[j * n for j in range(rows)])
    length = (ctypes.c_int32 * rows)(*[n] * rows)
    s = torch.cuda.current_stream(eng.device).cuda_stream
    dst = eng.wave[:rows]

    def kernel():
        _lib.call("tw_gather_windows", arena.data_ptr(), arena.numel(), start, length, rows, CHUNK, dst.data_ptr(),
                  eng.wave.stride(0), s)

    def slices():
        for j in range(rows):
            dst[j, :n].copy_(arena[j * n: (j + 1) * n], non_blocking=True)
            dst[j, n:].zero_()

    slices()
    ref = dst.clone()
    dst.fill_(-1.0)
    kernel()
    same = bool(torch.equal(dst, ref))
    us_k = device_us(kernel, a.reps, a.runs, a.warmup)
    us_s = device_us(slices, max(1, a.reps // 10), a.runs, a.warmup)
    nbytes = 4 * (rows * n + rows * CHUNK)
    return {"rows": rows, "window_seconds": seconds, "bytes": nbytes, "gather_us": us_k, "slices_us": us_s,
            "slice_launches": 2 * rows, "gather_tb_s": nbytes / us_k * 1e-6, "slices_tb_s": nbytes / us_s * 1e-6,
            "copy_rate_tb_s": COPY_RATE_TBS, "same_bytes": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[24, 96])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--model", default="large-v3-turbo")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_input_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multi_input_time.py needs the GPU: nothing is measured without one")
    tr = TurboTranscriber.from_pretrained(a.model, seed=1234, max_batch=24, device="cuda:0", max_beams=1)
    doc = {"model": a.model, "runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "gather": [gather_vs_slices(tr, sec, a) for sec in (30.0, 20.0)], "list_vs_loop": []}
    for n in a.clips:
        doc["list_vs_loop"].append(list_vs_loop(tr, n, a))
        print(json.dumps(doc["list_vs_loop"][-1]), flush=True)
    for g in doc["gather"]:
        print(json.dumps(g), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
