"""The list call on the CPU: TurboTranscriber.__call__(list) over a stand-in engine (flat window list, shared engine
batches, per-input stitching, errors, diagnostics), under a 2-rank gloo group, against transformers' own list-call
outputs (tests/golden/multi.json) for the stitching, and AudioProcessingPipeline.transcribe_many.

The engine needs the GPU, so each window's tokens are a deterministic function of the samples load() put into its
row of engine.wave: a window decodes to the same tokens in whatever batch it runs."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from twamd import audio
from twamd import audio_pipeline as ap
from twamd import dist as twd
from twamd import pipeline as tp
from twamd.config import GenerationSettings, PRESETS
from twamd.frontend import chunk_windows, time_precision
from twamd.pipeline import TurboTranscriber
from twamd.tokenizer import WhisperVocab, decode_asr

G = os.path.join(os.path.dirname(__file__), "golden")
ST = GenerationSettings.default(PRESETS["large-v3-turbo"]).special
SR = 16000


def _row_tokens(row):
    """<ts> text... <ts> from one 30-s row of samples."""
    h = int(abs(float(row[::997].sum())) * 1000) % 5000
    return [ST.timestamp_begin] + [300 + (h + 37 * i) % 20000 for i in range(1 + h % 7)] \
        + [ST.timestamp_begin + 50 + h % 1400]


class _FakeEngine:
    """WhisperEngine's surface as TurboTranscriber.transcribe_windows drives it: run_batches with load(k) filling
    wave[:n]; `sizes` records every run_batches call's batch sizes."""

    def __init__(self, max_batch):
        self.max_batch = max_batch
        self.wave = torch.zeros(max_batch, 480000)
        self.gen = GenerationSettings.default(PRESETS["large-v3-turbo"])
        self.device = torch.device("cpu")
        self.sizes = []
        self.kwargs = []

        class d:
            max_source_positions = 1500
        self.d = d

    def run_batches(self, sizes, load=None, batch_kwargs=None, **kw):
        out, self.batch_langs, self.batch_passes, self.batch_prefixes = [], [], [], []
        for k, n in enumerate(sizes):
            load(k)
            toks = [_row_tokens(r) for r in self.wave[:n].numpy()]
            out.append(toks)
            self.batch_langs.append([None] * n)
            self.batch_passes.append([[t] for t in toks])
            self.batch_prefixes.append([[None] for _ in toks])
        self.sizes.append(list(sizes))
        self.kwargs.append(kw)
        return out


def _tr(max_batch=8):
    eng = _FakeEngine(max_batch)
    return TurboTranscriber(eng, WhisperVocab.synthetic(ST)), eng


def _inputs():
    """3 windows, a 7-s input, 5 windows with a ragged last one (at chunk 30 / stride 0)."""
    rng = np.random.default_rng(5)
    return [rng.standard_normal(n).astype(np.float32) for n in (90 * SR, 7 * SR, 131 * SR)]


def _kw(**over):
    kw = dict(chunk_length_s=30, stride_length_s=0, batch_size=24, return_timestamps=True,
              generate_kwargs={"task": "transcribe", "num_beams": 1, "max_new_tokens": 128, "max_passes": 1})
    kw.update(over)
    return kw


def _singles(xs, kw):
    out, passes = [], []
    for x in xs:
        tr, _ = _tr()
        out.append(tr(x, **kw))
        passes.append(tr.last_window_passes)
    return out, passes


def test_list_call_equals_single_calls_and_shares_batches():
    xs = _inputs()
    tr, eng = _tr(8)
    got = tr(xs, **_kw())
    ref, _ = _singles(xs, _kw())
    assert isinstance(got, list) and got == ref
    assert all(len(r["chunks"]) > 0 for r in got)
    assert eng.sizes == [[5, 4]]  # 9 windows of the call in two near-equal batches, not three calls' batches


def test_list_call_with_strides_keeps_every_inputs_own_strides(monkeypatch):
    xs = _inputs()
    kw = _kw(stride_length_s=5)
    ref, _ = _singles(xs, kw)
    seen = []
    monkeypatch.setattr(tp, "decode_asr", lambda vocab, outputs, **k: (seen.append([o["stride"] for o in outputs]),
                                                                       decode_asr(vocab, outputs, **k))[1])
    tr, eng = _tr(8)
    assert tr(xs, **kw) == ref
    own = [[(w.length / SR, w.stride_left / SR, w.stride_right / SR) for w in chunk_windows(len(x), 30, 5, SR)]
           for x in xs]
    assert seen == own  # one decode_asr per input, with the input's own stride triples (no arena offsets)
    assert [len(s) for s in own] == [4, 1, 7] and eng.sizes == [[6, 6]]


def test_grouped_mode_groups_cross_input_boundaries():
    """Where batch composition shapes results (here condition_on_prev_tokens, which the stand-in ignores), the
    engine batches are batch_size-sized groups over the flat window list, as the DataLoader's batches are."""
    xs = _inputs()
    kw = _kw(batch_size=4)
    kw["generate_kwargs"] = dict(kw["generate_kwargs"], condition_on_prev_tokens=True)
    tr, eng = _tr(8)
    got = tr(xs, **kw)
    assert eng.sizes == [[4, 4, 1]]  # 3 + 1 + 5 windows: the second group holds windows of all three inputs
    assert eng.kwargs[0].get("condition_on_prev_tokens") is True
    assert got == _singles(xs, kw)[0]


def test_no_chunking_short_inputs_share_a_batch_and_long_ones_run_alone():
    rng = np.random.default_rng(6)
    short1, long, short2 = (rng.standard_normal(n).astype(np.float32) for n in (12 * SR, 75 * SR, 20 * SR))
    tr, eng = _tr(8)
    seen = []

    def long_form(wav, **kw):
        seen.append((np.asarray(wav).copy(), list(eng.sizes)))
        return {"text": "LONG", "chunks": []}

    tr._long_form = long_form
    kw = _kw(chunk_length_s=0)
    got = tr([short1, long, short2], **kw)
    assert len(seen) == 1 and np.array_equal(seen[0][0], long)
    assert eng.sizes == [[2]]  # the two short inputs, one window each, in one batch
    ref, _ = _singles([short1, short2], kw)
    assert got == [ref[0], {"text": "LONG", "chunks": []}, ref[1]]
    assert tr.last_input_windows == [(0, 1), (1, 0), (1, 1)]  # (the stub left no record of its passes)


def test_list_call_errors(monkeypatch):
    xs = _inputs()
    tr, eng = _tr(8)
    assert tr([], **_kw()) == []
    with pytest.raises(ValueError, match=r"inputs\[1\] is empty"):
        tr([xs[1], np.zeros(0, np.float32), xs[1]], **_kw())
    with pytest.raises(TypeError, match=r"^inputs\[1\]: We expect a numpy ndarray"):
        tr([xs[1], object(), xs[1]], **_kw())
    with pytest.raises(ValueError, match=r"^inputs\[0\]: a dict input needs"):
        tr([{"raw": xs[1]}], **_kw())
    monkeypatch.setenv("TW_MAX_AUDIO_S", "60")
    with pytest.raises(ValueError, match="split the list"):
        tr([xs[1]] * 9, **_kw())  # 63 s
    assert len(tr([xs[1]] * 8, **_kw())) == 8  # 56 s
    monkeypatch.delenv("TW_MAX_AUDIO_S")
    with pytest.raises(TypeError, match="We expect a numpy ndarray or torch tensor as input"):
        tr((xs[1], xs[1]), **_kw())
    assert eng.sizes == [[8]]  # no refused call reached the engine


def test_diagnostics_line_up_with_the_results():
    xs = _inputs()
    tr, eng = _tr(8)
    got = tr(xs, **_kw())
    ref, passes = _singles(xs, _kw())
    assert tr.last_input_windows == [(0, 3), (3, 1), (4, 5)]
    assert len(tr.last_window_passes) == len(tr.last_window_langs) == len(tr.last_window_prefixes) == 9
    for (first, n), p, r, g in zip(tr.last_input_windows, passes, ref, got):
        assert tr.last_window_passes[first: first + n] == p and g == r


# ------------------------------------------------------------------------------------------------ gloo, 2 ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        tr, eng = _tr(8)
        xs = _inputs() if rank == 0 else [None] * 3
        out = tr(xs, **_kw(stride_length_s=5))
        try:  # a failed decode on rank 0 is collective: rank 0 raises its own error, the others PeerError
            tr([_inputs()[1], object()] if rank == 0 else [None] * 2, **_kw())
            err = None
        except twd.PeerError:
            err = "peer"
        except TypeError as e:
            err = str(e)[:10]
        sizes, spans = list(eng.sizes), tr.last_input_windows
        fe = twd.RankZeroFrontend(tr)  # serving: rank 0 passes the list through, the followers learn its length
        if rank == 0:
            served = fe(_inputs(), **_kw(stride_length_s=5))
            fe.close()
        else:
            served = fe.follow()
        q.put((rank, out, sizes, spans, err, served))
    finally:
        dist.destroy_process_group()


def test_two_rank_list_call_equals_single_process():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    tr, eng = _tr(8)
    ref = tr(_inputs(), **_kw(stride_length_s=5))
    assert eng.sizes == [[6, 6]]
    for rank, out, sizes, spans, err, served in res:
        assert out == ref  # every rank returns the whole list
        assert spans == [(0, 4), (4, 1), (5, 7)]
    assert res[0][5] == ref and res[1][5] == 1  # through RankZeroFrontend: rank 0's result, one call followed
    assert [r[2] for r in res] == [[[6]], [[6]]]  # 12 flat windows: each rank ran half of them
    assert [r[4] for r in res] == ["inputs[1]:", "peer"]


# ------------------------------------------------------------------------------------ transformers' list outputs
def test_decode_asr_input_by_input_reproduces_transformers_list_results():
    gold = json.load(open(os.path.join(G, "multi.json")))
    vocab = WhisperVocab.synthetic(GenerationSettings.default(PRESETS["test-mini"]).special)
    names = [c["name"] for c in gold["cases"]]
    assert names == ["chunk_30_5_b4", "ref_60_5_b32", "nochunk_short_b2", "nochunk_mixed_b1", "beam3_30_5_b4",
                     "word_30_5_b2"]
    for c in gold["cases"]:
        assert len(c["windows"]) == len(c["list_output"]) == len(c["inputs"])
        for outs, ref in zip(c["windows"], c["list_output"]):
            outs = [dict(o, **({"stride": tuple(o["stride"])} if "stride" in o else {})) for o in outs]
            text, optional = decode_asr(vocab, outs, return_timestamps=c["return_timestamps"],
                                        time_precision=time_precision(1500))
            assert json.loads(json.dumps({"text": text, **optional})) == ref, c["name"]


# ----------------------------------------------------------------------------------------------- transcribe_many
class FakeASR:
    def __init__(self, exc=None):
        self.calls = []
        self.exc = exc

    def __call__(self, inputs, **kw):
        self.calls.append((inputs, kw))
        if self.exc:
            raise self.exc
        return [{"text": f" {len(x)}"} for x in inputs]


def _wav(tmp_path, name, seconds):
    p = str(tmp_path / name)
    audio.write_wav(p, np.zeros(int(SR * seconds), np.float32))
    return p


def test_transcribe_many(tmp_path):
    a, b = _wav(tmp_path, "a.wav", 3.0), _wav(tmp_path, "b.wav", 2.0)
    missing = str(tmp_path / "missing.wav")
    f = FakeASR()
    pipe = ap.AudioProcessingPipeline(transcriber=f)
    out = pipe.transcribe_many([a, missing, b], task="translate")
    assert out[0] == {"text": " 48000"} and out[2] == {"text": " 32000"}
    assert set(out[1]) == {"error"} and out[1]["error"].startswith("Transcription error: ")
    (inp, kw), = f.calls  # one list call, with the reference's arguments
    assert [len(x) for x in inp] == [48000, 32000]
    assert kw == {"chunk_length_s": 60, "batch_size": 512 if pipe.gpu_available else 32, "stride_length_s": 5,
                  "generate_kwargs": {"task": "translate"}, "return_timestamps": True}
    bad = ap.AudioProcessingPipeline(transcriber=FakeASR(exc=RuntimeError("boom")))
    assert bad.transcribe_many([a, missing, b])[0] == {"error": "Transcription error: boom"}
    assert all(set(r) == {"error"} for r in bad.transcribe_many([a, missing, b]))
    none = FakeASR()
    assert ap.AudioProcessingPipeline(transcriber=none).transcribe_many([]) == [] and none.calls == []
