"""The list call on the MI355X (test-mini, seeded weights): tw_gather_windows against torch slicing, its host-side
refusals, TurboTranscriber.__call__(list) against the single calls (exactly: rows do not depend on their batch)
and against transformers' own list-call outputs (tests/golden/multi.json), the batch schedule, and the sharded
single-input device path, whose per-window slice copies the kernel replaced.

Tolerances: the kernel is a copy (torch.equal). List call vs single calls: exact. Against transformers: the result
equals the golden, or every device decision replays within TAU = 0.3 logits on the fp32 oracle, as
tests/test_gpu_e2e.py::test_pipeline_matches_transformers_pipeline judges it; word times as tests/test_gpu_word.py
(|diff| <= 0.2 s, >= 90 % equal)."""
import ctypes
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist

from oracle import whisper_oracle as wo
from twamd import _lib
from twamd import dist as twd
from twamd.config import PRESETS, GenerationSettings
from twamd.frontend import chunk_windows
from twamd.pipeline import TurboTranscriber, batch_sizes

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
D = PRESETS["test-mini"]
DEV = "cuda"
HEADS = [(1, 0), (1, 1), (1, 2), (1, 3)]
TAU = 0.3  # tests/test_gpu_e2e.py::test_pipeline_matches_transformers_pipeline's
SENTINEL = -7.0


def S():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------------ the kernel
def _gather(arena, start, length, rows, row_len, out, out_stride, arena_len=None):
    n = len(start)
    st = (ctypes.c_int64 * max(n, 1))(*start)
    ln = (ctypes.c_int32 * max(n, 1))(*length)
    rc = _lib.load().tw_gather_windows(arena.data_ptr(), arena.numel() if arena_len is None else arena_len, st, ln,
                                       rows, row_len, out.data_ptr(), out_stride, S())
    torch.cuda.synchronize()
    return rc


def _arena(n, pad):
    """n finite random floats in the middle of a larger tensor whose neighbours hold NaN; pad = floats before it
    (the allocation is 256-byte aligned: pad 4 keeps the arena 16-byte aligned, pad 3 does not)."""
    big = torch.full((pad + n + 5,), float("nan"), device=DEV)
    big[pad: pad + n] = torch.randn(n, generator=torch.Generator().manual_seed(n + pad)).to(DEV)
    return big[pad: pad + n]


def _check(arena, start, length, row_len, out_stride, out_off=0):
    rows = len(start)
    buf = torch.full((out_off + (rows + 2) * out_stride,), SENTINEL, device=DEV)
    out = buf[out_off:].view(rows + 2, out_stride)
    ref = out.clone()
    for j in range(rows):
        ref[j, :row_len] = 0
        ref[j, : length[j]] = arena[start[j]: start[j] + length[j]]
    assert _gather(arena, start, length, rows, row_len, out, out_stride) == 0, _lib.load().tw_last_error()
    assert not torch.isnan(out).any()
    assert torch.equal(out, ref)  # (the sentinel in out[j][row_len:] and in the rows past `rows` included)
    assert (buf[:out_off] == SENTINEL).all()


@pytest.mark.parametrize("pad", [4, 3], ids=["arena16", "arena4"])
@pytest.mark.parametrize("out_off", [0, 1], ids=["out16", "out4"])
def test_gather_edges(pad, out_off):
    """An empty row, a one-sample row, a full row that ends at the arena's last element, a row length that is no
    multiple of 4; sources and outputs that are and are not 16-byte aligned."""
    n = 4096 + 3
    _check(_arena(n, pad), [0, 5, n - 1003], [0, 1, 1003], 1003, 1004, out_off)
    _check(_arena(n, pad), [1, 2, 4, 8], [1003, 1002, 1001, 7], 1003, 1004, out_off)


def test_gather_more_rows_than_one_launch():
    rng = np.random.default_rng(65)
    length = [int(x) for x in rng.integers(0, 65, size=65)]
    length[0], length[63], length[64] = 64, 64, 63
    start = [int(rng.integers(0, 5000 - n + 1)) for n in length]
    _check(_arena(5000, 4), start, length, 64, 64)


def test_gather_real_shape():
    _check(_arena(960001, 4), [1, 480001], [480000, 480000], 480000, 480000)


def test_gather_refusals():
    """Host-side checks: nothing is launched, out keeps its sentinel."""
    arena = _arena(2048, 4)
    out = torch.full((4, 104), SENTINEL, device=DEV)
    lib = _lib.load()
    for what, args, kw in [
        ("negative start", ([0, -1], [100, 100], 2, 100, out, 104), {}),
        ("start + length > arena_len", ([0, 1949], [100, 100], 2, 100, out, 104), {}),
        ("length > row_len", ([0, 10], [100, 101], 2, 100, out, 104), {}),
        ("negative length", ([0, 10], [100, -1], 2, 100, out, 104), {}),
        ("row_len > out_stride", ([0, 10], [100, 100], 2, 105, out, 104), {}),
        ("rows < 0", ([0], [100], -1, 100, out, 104), {}),
        ("a bad row past the first launch", ([0] * 70, [100] * 69 + [101], 70, 100,
                                             torch.full((70, 104), SENTINEL, device=DEV), 104), {}),
    ]:
        assert _gather(arena, *args, **kw) != 0, what
        assert b"tw_gather_windows" in lib.tw_last_error(), what
        assert (args[4] == SENTINEL).all(), what
    with pytest.raises(_lib.TwError, match="exceeds arena_len"):
        st, ln = (ctypes.c_int64 * 1)(2000), (ctypes.c_int32 * 1)(100)
        _lib.call("tw_gather_windows", arena.data_ptr(), 2048, st, ln, 1, 100, out.data_ptr(), 104, S())


# ---------------------------------------------------------------------------------------------------- the callable
@pytest.fixture(scope="module")
def tr():
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=4)
    t.engine.gen.alignment_heads = list(HEADS)
    return t


@pytest.fixture(scope="module")
def oracle():
    sd = wo.synth_state_dict(D.d_model, D.encoder_layers, D.decoder_layers, D.ffn, D.n_mels, D.vocab, 1234)
    return wo.WhisperOracle(sd, D.heads)


@pytest.fixture(scope="module")
def clips():
    sys.path.insert(0, G)
    from make_golden_multi import inputs
    return {k: np.ascontiguousarray(v, np.float32) for k, v in inputs().items()}


def _gcfg():
    gen = GenerationSettings.default(D)
    st = gen.special
    return wo.GenCfg(D.vocab, st.eot, st.sot, st.lang_begin, st.n_languages, st.transcribe, st.translate,
                     st.notimestamps, gen.suppress_tokens, gen.begin_suppress_tokens)


GREEDY = {"task": "transcribe", "num_beams": 1, "max_new_tokens": 24}
EQUAL_CASES = {  # name: (inputs, call kwargs)
    "chunk_30_5": (("mix75", "noise12", "speech45"),
                   dict(chunk_length_s=30, stride_length_s=5, batch_size=4, return_timestamps=True,
                        generate_kwargs=GREEDY)),
    "reference_call": (("mix75", "noise12", "speech45"),
                       dict(chunk_length_s=60, stride_length_s=5, batch_size=32, return_timestamps=True,
                            generate_kwargs={"task": "transcribe", "max_new_tokens": 16})),
    "nochunk_short": (("noise12", "mix20"), dict(batch_size=2, return_timestamps=True, generate_kwargs=GREEDY)),
    "nochunk_mixed": (("mix75", "noise12"), dict(batch_size=1, return_timestamps=True, generate_kwargs=GREEDY)),
    # 4 + 2 + 1 windows at batch_size 2: every input's windows are whole groups of their own in both forms
    "word_conf_alt": (("mix75", "speech45", "noise12"),
                      dict(chunk_length_s=30, stride_length_s=5, batch_size=2, return_timestamps="word",
                           return_confidence=True, return_alternatives=2, generate_kwargs=GREEDY)),
}


@pytest.mark.parametrize("name", list(EQUAL_CASES))
def test_list_call_equals_single_calls_exactly(tr, clips, name):
    names, kw = EQUAL_CASES[name]
    got = tr([clips[n] for n in names], **kw)
    passes, langs, spans = tr.last_window_passes, tr.last_window_langs, tr.last_input_windows
    assert isinstance(got, list) and len(got) == len(names) and len(spans) == len(names)
    for n, r, (first, count) in zip(names, got, spans):
        single = tr(clips[n], **kw)
        assert r == single, (name, n)
        assert passes[first: first + count] == tr.last_window_passes, (name, n)
        assert langs[first: first + count] == tr.last_window_langs, (name, n)
    assert spans[-1][0] + spans[-1][1] == len(passes)


def _close_times(got, ref, what):  # tests/test_gpu_word.py's bound
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, what
    if got.size == 0:
        return
    d = np.abs(got - ref)
    assert d.max() <= 0.2 + 1e-6, (what, float(d.max()))
    assert (d < 1e-6).mean() >= 0.9, (what, float((d < 1e-6).mean()))


def _beam_passes_within_tau(passes, langs, oracle, segs, max_new, num_beams):
    """tests/test_gpu_e2e.py's judgement of beam passes: equal to the fp32 oracle's beam search (pinned to
    transformers) until the first pass that differs, whose first differing decision must be one the fp32 search
    could make within tolerance."""
    g = _gcfg()
    for k, seg_audio in enumerate(segs):
        feats = wo.log_mel(seg_audio, D.n_mels)
        prompt = [g.sot, int(langs[k]), g.transcribe]
        seek = 0
        for raw in passes[k]:
            seg = np.zeros_like(feats)
            seg[:, : 3000 - seek] = feats[:, seek:]
            enc = oracle.encode(seg)
            ora = wo.beam_pass(oracle, enc, prompt, max_new, g, True, num_beams)
            dev = [int(x) for x in raw]
            dev = dev[: dev.index(g.eot) + 1] if g.eot in dev else dev
            if ora != dev:
                tdiv = next((i for i in range(min(len(ora), len(dev))) if ora[i] != dev[i]), min(len(ora), len(dev)))
                if tdiv < len(dev):
                    cache = oracle.new_cache(enc)
                    for tok in prompt[:-1]:
                        oracle.decoder_step(tok, cache)
                    lg = oracle.decoder_step(prompt[-1], cache)
                    for tok in dev[:tdiv]:
                        lg = oracle.decoder_step(tok, cache)
                    lsm = wo._log_softmax32(lg)
                    proc = wo.process_logits(lsm, dev[:tdiv], g, True)
                    cands = set(int(x) for x in np.argsort(-proc, kind="stable")[: 2 * num_beams])
                    assert dev[tdiv] in cands or wo.decision_ok(lsm, dev[:tdiv], g, True, dev[tdiv], TAU), \
                        (k, seek, tdiv, "oracle", ora, "device", dev)
                break
            seq = dev[:-1] if dev and dev[-1] == g.eot else dev
            _, off = wo.retrieve_segment(seq, 3000 - seek, g.ts_begin)
            seek += off


@pytest.mark.parametrize("name", ["chunk_30_5_b4", "ref_60_5_b32", "nochunk_short_b2", "nochunk_mixed_b1",
                                  "beam3_30_5_b4", "word_30_5_b2"])
def test_list_call_matches_transformers_list_call(tr, oracle, clips, name, monkeypatch):
    """Every input's result equals transformers' (the list call of tests/golden/multi.json), or every device
    decision of that input's windows is one the fp32 reference could make within TAU (a window whose tokens are
    the golden's made transformers' own decisions and is not replayed)."""
    from twamd import pipeline as tp
    from twamd.tokenizer import decode_asr
    stitched = []  # per decode_asr call (the chunked / short inputs in order, then the long-form ones) its tokens
    monkeypatch.setattr(tp, "decode_asr", lambda vocab, outputs, **k: (
        stitched.append([list(o["tokens"]) for o in outputs]), decode_asr(vocab, outputs, **k))[1])
    gold = json.load(open(os.path.join(G, "multi.json")))
    c = next(x for x in gold["cases"] if x["name"] == name)
    kw = dict(c["kwargs"])
    if "batch_size" in kw:  # (groups matter for the word case only; its batch_size 2 fits the engine)
        kw["batch_size"] = min(kw["batch_size"], tr.engine.max_batch)
    gk = {"task": "transcribe", "num_beams": 1, "max_new_tokens": gold["max_new_tokens"], **c["generate_kwargs"]}
    xs = [clips[n] for n in c["inputs"]]
    got = tr(xs, generate_kwargs=dict(gk), return_timestamps=c["return_timestamps"], **kw)
    assert len(got) == len(c["list_output"])
    g = _gcfg()
    word = c["return_timestamps"] == "word"
    longs = [i for i, x in enumerate(xs) if not kw.get("chunk_length_s") and len(x) > 480000]
    tokens = dict(zip([i for i in range(len(xs)) if i not in longs] + longs, stitched))

    def unpadded(t):
        t = [int(v) for v in t]
        while t and t[-1] == g.eot:
            t.pop()
        return t

    for i, (x, r, ref) in enumerate(zip(xs, got, c["list_output"])):
        first, count = tr.last_input_windows[i]
        passes = tr.last_window_passes[first: first + count]
        langs = tr.last_window_langs[first: first + count]
        if word and r["text"] == ref["text"]:
            assert [w["text"] for w in r["chunks"]] == [w["text"] for w in ref["chunks"]], (name, i)
            _close_times([t for w in r["chunks"] for t in w["timestamp"]],
                         [t for w in ref["chunks"] for t in w["timestamp"]], (name, i))
            print(f"{name} input {i}: text exact, word times within the bound")
            continue
        if not word and json.loads(json.dumps(r)) == ref:
            print(f"{name} input {i}: exact")
            continue
        print(f"{name} input {i}: differs from transformers, checking every decision")
        cl = kw.get("chunk_length_s", 0)
        if cl:
            segs = [x[w.start: w.start + min(w.length, 480000)]
                    for w in chunk_windows(len(x), cl, kw.get("stride_length_s"), 16000)]
        elif len(x) > 480000:
            segs = None  # long-form: one record, replayed over the whole input's frames
        else:
            segs = [x]
        if segs is None:
            f = wo.log_mel(x, D.n_mels, long=True)
            assert count == 1
            st = wo.replay_generate(oracle, f, g, passes[0], langs[0], max_new_tokens=gk["max_new_tokens"], tau=TAU,
                                    max_frames=f.shape[1])
            assert st["ok"], (name, i, st)
            continue
        assert len(segs) == count == len(tokens[i]) == len(c["windows"][i])
        differ = [k for k in range(count) if unpadded(tokens[i][k]) != unpadded(c["windows"][i][k]["tokens"])]
        assert differ, (name, i)
        print(f"{name} input {i}: windows {differ} of {count} differ")
        passes, langs, segs = ([v[k] for k in differ] for v in (passes, langs, segs))
        if gk["num_beams"] > 1:
            _beam_passes_within_tau(passes, langs, oracle, segs, gk["max_new_tokens"], gk["num_beams"])
            continue
        for k, seg in enumerate(segs):
            st = wo.replay_generate(oracle, wo.log_mel(seg, D.n_mels), g, passes[k], langs[k],
                                    max_new_tokens=gk["max_new_tokens"], tau=TAU)
            assert st["ok"], (name, i, k, st)


def test_schedule_one_gather_per_engine_batch(tr, clips, monkeypatch):
    """7 windows at max_batch 4: the batches batch_sizes() gives for the call's windows together, and one
    tw_gather_windows launch per batch (the arena stays in device memory)."""
    names, kw = EQUAL_CASES["chunk_30_5"]
    calls = []
    orig = _lib.call

    def counting(fn, *a):
        calls.append(fn)
        return orig(fn, *a)

    monkeypatch.setattr(_lib, "call", counting)
    tr([clips[n] for n in names], **kw)
    total = sum(n for _, n in tr.last_input_windows)
    sizes = batch_sizes(total, tr.engine.max_batch, tr.sub_batch_min)
    assert total == 7 and sizes == [4, 3]
    assert [len(p) for p in tr.engine.batch_passes] == sizes
    assert calls.count("tw_gather_windows") == len(sizes)


@pytest.fixture(scope="module")
def rccl_group():
    assert not dist.is_initialized()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    yield dev
    dist.destroy_process_group()


def test_sharded_device_path_gathers_and_equals_plain_call(tr, clips, rccl_group, monkeypatch):
    """A forced collective in a world of one: the single input is broadcast into device memory and its windows are
    gathered out of it by the kernel (no per-window slice copies); tokens and result equal the plain call's. The
    list call through the same collectives equals the plain list call."""
    kw = EQUAL_CASES["chunk_30_5"][1]
    x = clips["mix75"]
    plain = tr(x, **kw)
    plain_passes = tr.last_window_passes
    xs = [clips[n] for n in EQUAL_CASES["chunk_30_5"][0]]
    plain_list = tr(xs, **kw)
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (calls.append(fn), orig(fn, *a))[1])
    monkeypatch.setattr(twd, "FORCE_COLLECTIVE", True)
    assert twd.collective_path()
    assert tr(x, **kw) == plain
    assert tr.last_window_passes == plain_passes
    assert calls.count("tw_gather_windows") == 1  # 4 windows, one batch
    assert tr(xs, **kw) == plain_list
