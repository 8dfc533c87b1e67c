"""Forced alignment on the GPU: tw_logits_force against a few lines of Python and float64 log_softmax,
tw_align_cost against the float64 cost matrix of the same f32 probabilities (tests/align_ref.py), and
WhisperEngine.force_pass / TurboTranscriber.align on test-mini against the oracle fed the same tokens.

Bounds. Log-probabilities: 1e-4 absolute for the kernel alone (f32 logsumexp, tests/test_gpu_confidence.py's bound for
tw_token_logprob); through the bf16 engine 0.30 per token and 0.03 in a row's mean (that file's bf16 bounds), through
the fp32 engine 1e-3. Cost matrices: the kernel may be 4 x as far from float64 as the host's own f32 arithmetic
(twamd.alignment) on the same input — another summation order; the median is 1-Lipschitz, so the standardisation
error is the whole error. Times: tests/test_gpu_word.py's rule, every |d| <= 0.2 s and >= 90 % exactly equal."""
import numpy as np
import pytest
import torch

import align_ref as ar
from oracle import whisper_oracle as wo
from twamd import _lib, alignment
from twamd.config import PRESETS
from twamd.pipeline import TurboTranscriber
from twamd.synth_audio import speech_like, white_noise
from twamd.tokenizer import collate_word_timestamps

pytestmark = pytest.mark.gpu
D = PRESETS["test-mini"]
DEV = "cuda"
HEADS = [(1, 0), (1, 1), (1, 2), (1, 3)]
ST = _lib.TW_STATE_STRIDE


def S():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- tw_logits_force
@pytest.mark.parametrize("extra", [0, 37])
def test_logits_force_vs_torch(extra):
    B, V, ld = 3, D.vocab, D.vocab + extra
    pad, ld_tok, ld_lp, ld_force = 50257, 8, 7, 6
    flen = [0, 1, 5]
    g = torch.Generator(device="cpu").manual_seed(17 + extra)
    force_h = torch.randint(0, V, (B, ld_force), generator=g, dtype=torch.int32)
    force, force_len = force_h.to(DEV), torch.tensor(flen, dtype=torch.int32, device=DEV)
    state = torch.zeros(B, ST, dtype=torch.int32, device=DEV)
    state[:, _lib.TW_ST_LAST:_lib.TW_ST_LASTTS + 1] = -1
    tokens = torch.full((B, ld_tok), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((B, ld_lp), float("nan"), dtype=torch.float32, device=DEV)
    ids = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    pos = torch.tensor([3, 4, 5], dtype=torch.int32, device=DEV)
    # the same in Python
    e_tok, e_lp = np.full((B, ld_tok), -7, np.int64), np.full((B, ld_lp), np.nan)
    ngen, last, pen, fin, e_pos = [0] * B, [-1] * B, [-1] * B, [0] * B, [3, 4, 5]
    for call in range(6):
        lg_h = torch.randn(B, ld, generator=g) * 3.0
        lg_h[:, V:] = float("inf")  # pad columns: never read
        lg = lg_h.to(DEV)
        _lib.call("tw_logits_force", lg.data_ptr(), B, ld, V, force.data_ptr(), ld_force, force_len.data_ptr(), pad,
                  state.data_ptr(), tokens.data_ptr(), ld_tok, ids.data_ptr(), pos.data_ptr(), lp.data_ptr(), ld_lp,
                  S())
        torch.cuda.synchronize()
        e_ids = []
        for b in range(B):
            n = ngen[b]
            if n < flen[b]:
                tok = int(force_h[b, n])
                e_tok[b, n] = tok
                e_lp[b, n] = torch.log_softmax(lg_h[b, :V].double(), -1)[tok].item()
                pen[b], last[b], ngen[b] = last[b], tok, n + 1
                e_ids.append(tok)
            else:
                fin[b] = 1
                e_ids.append(pad)
                e_tok[b, n], e_lp[b, n] = pad, 0.0
            e_pos[b] += 1
        st = state.cpu().numpy()
        assert st[:, _lib.TW_ST_NGEN].tolist() == ngen and st[:, _lib.TW_ST_FINISHED].tolist() == fin, call
        assert st[:, _lib.TW_ST_LAST].tolist() == last and st[:, _lib.TW_ST_PENULT].tolist() == pen, call
        assert ids.tolist() == e_ids and pos.tolist() == e_pos, call
        assert np.array_equal(tokens.cpu().numpy(), e_tok), call
        got = lp.cpu().numpy().astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(e_lp)), call  # nothing else written
        m = ~np.isnan(e_lp)
        err = np.abs(got[m] - e_lp[m]).max() if m.any() else 0.0
        assert err <= 1e-4, (call, err)
    # past a row's end: the pad token and 0.0 at the row's length, and the row stays there
    assert ngen == flen and fin == [1, 1, 1]
    for b in range(B):
        assert e_tok[b, flen[b]] == pad and e_lp[b, flen[b]] == 0.0


def test_logits_force_refuses_bad_arguments():
    lib = _lib.load()
    B, V = 2, 128
    i32 = dict(dtype=torch.int32, device=DEV)
    lg = torch.zeros(B, V, device=DEV)
    force, flen, state = torch.zeros(B, 4, **i32), torch.ones(B, **i32), torch.zeros(B, ST, **i32)
    tok, ids, pos, lp = torch.zeros(B, 4, **i32), torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(B, 4, device=DEV)
    ok = [lg.data_ptr(), B, V, V, force.data_ptr(), 4, flen.data_ptr(), 0, state.data_ptr(), tok.data_ptr(), 4,
          ids.data_ptr(), pos.data_ptr(), lp.data_ptr(), 4, S()]
    for i in (0, 4, 6, 8, 9, 11, 13):  # every required pointer
        bad = list(ok)
        bad[i] = None
        assert lib.tw_logits_force(*bad) != 0, i
    bad = list(ok)
    bad[2] = V - 1  # V > ld_logits
    assert lib.tw_logits_force(*bad) != 0
    torch.cuda.synchronize()
    assert state.sum().item() == 0  # nothing ran
    assert lib.tw_logits_force(*ok[:12], None, *ok[13:]) == 0  # pos may be NULL
    torch.cuda.synchronize()
    # the TW_DEBUG build checks the forced id the launch is about to commit
    dbg = _lib.load_debug()
    state.zero_()
    force[1, 0] = V
    assert dbg.tw_logits_force(*ok) != 0 and b"forced id" in dbg.tw_last_error()
    torch.cuda.synchronize()
    assert state.sum().item() == 0
    force[1, 0] = V - 1
    assert dbg.tw_logits_force(*ok) == 0
    torch.cuda.synchronize()
    assert state[:, _lib.TW_ST_NGEN].tolist() == [1, 1]


# ---------------------------------------------------------------- tw_align_cost
def _probs(rng, B, n_steps, n_slots, Sx):
    """Attention-like f32 probabilities: per (row, step, slot) a bump that moves with the step, plus noise."""
    f = np.arange(Sx, dtype=np.float64)[None, None, None, :]
    centre = (np.arange(n_steps)[None, :, None, None] + 0.5) * Sx / n_steps + rng.normal(0, 3, (B, n_steps, n_slots, 1))
    w = np.exp(-0.5 * ((f - centre) / 12.0) ** 2) + 0.05 * rng.random((B, n_steps, n_slots, Sx))
    return (w / w.sum(-1, keepdims=True)).astype(np.float32)


def _host32_cost(w, width):
    """twamd.alignment's own arithmetic on w f32 [slots][rows][frames]: token_timestamps' f32 standardisation and
    median_filter, head mean, negated."""
    with np.errstate(invalid="ignore", divide="ignore"):
        z = ((w - w.mean(axis=-2, keepdims=True)) / w.std(axis=-2, keepdims=True)).astype(np.float32)
    return -alignment.median_filter(z, width).mean(axis=0)


def _run_align_cost(p, n_rows, n_frames, width):
    B, n_steps, n_slots, Sx = p.shape
    probs = torch.from_numpy(p).to(DEV)
    cost = torch.full((B, n_steps, Sx), float("nan"), dtype=torch.float32, device=DEV)
    nr = torch.tensor(n_rows, dtype=torch.int32, device=DEV)
    nf = torch.tensor(n_frames, dtype=torch.int32, device=DEV)
    _lib.call("tw_align_cost", probs.data_ptr(), B, n_steps, n_slots, Sx, nr.data_ptr(), nf.data_ptr(), width,
              cost.data_ptr(), S())
    torch.cuda.synchronize()
    return cost.cpu().numpy()


def _check_align_cost(p, n_rows, n_frames, width, what, base=None):
    """base: the probabilities before constant columns were planted in p. The host's own f32 error is taken there:
    on a planted column its f32 mean is not the value, so its z is finite garbage where float64 (and the kernel)
    have NaN, which would inflate the bound."""
    got = _run_align_cost(p, n_rows, n_frames, width)
    base = p if base is None else base
    worst = 0.0
    for b, (nr, nf) in enumerate(zip(n_rows, n_frames)):
        if nr < 2:
            assert np.isnan(got[b]).all(), (what, b, "a row of one token is left untouched")
            continue
        assert np.isnan(got[b, nr:]).all() and np.isnan(got[b, :, nf:]).all(), (what, b, "written outside its extent")
        w = np.ascontiguousarray(p[b, :nr, :, :nf].transpose(1, 0, 2))  # [slots][rows][frames]
        ref = ar.cost_matrix(w, width, np.float64)
        w0 = np.ascontiguousarray(base[b, :nr, :, :nf].transpose(1, 0, 2))
        g = got[b, :nr, :nf]
        assert np.array_equal(np.isnan(g), np.isnan(ref)), (what, b, "NaN positions")
        m = np.isfinite(ref)
        e_gpu = float(np.abs(g[m].astype(np.float64) - ref[m]).max())
        e_host = float(np.abs(_host32_cost(w0, width).astype(np.float64) - ar.cost_matrix(w0, width, np.float64)).max())
        print(f"tw_align_cost {what} row {b} (n_rows {nr}, n_frames {nf}, width {width}): |gpu - f64| {e_gpu:.3g}, "
              f"|host f32 - f64| {e_host:.3g}, ratio {e_gpu / e_host if e_host else float('inf'):.2f}")
        assert e_gpu <= 4.0 * e_host, (what, b, e_gpu, e_host)
        worst = max(worst, e_gpu)
    return got, worst


@pytest.mark.parametrize("n_steps,n_slots,n_rows,n_frames", [
    (5, 1, [1, 2, 5], [613, 3, 1500]),
    (5, 4, [3, 5, 2], [4, 7, 1500]),
    (127, 6, [127, 3, 5], [1500, 613, 7]),
    (127, 6, [2, 1, 127], [4, 1500, 613]),
])
def test_align_cost_vs_float64(n_steps, n_slots, n_rows, n_frames):
    B, Sx = 3, 1500
    p = _probs(np.random.default_rng(n_steps * 10 + n_slots + n_rows[0]), B, n_steps, n_slots, Sx)
    planted, base = [], p.copy()
    for b in range(B):  # a constant column per row (its z is NaN), and a run of four where a window can hold them
        col = min(2, n_frames[b] - 1) if n_frames[b] < 20 else n_frames[b] // 3
        p[b, :, n_slots - 1, col] = np.float32(0.3)  # (0.3f: sums of it are not exact in f32)
        planted.append(col)
        if n_frames[b] >= 20:
            p[b, :, 0, col + 50: col + 54] = np.float32(0.7)
    got, _ = _check_align_cost(p, n_rows, n_frames, 7, f"{n_steps}x{n_slots}", base)
    for b in range(B):
        if n_rows[b] < 2:
            continue
        nr, nf, col = n_rows[b], n_frames[b], planted[b]
        ref = ar.cost_matrix(np.ascontiguousarray(p[b, :nr, :, :nf].transpose(1, 0, 2)), 7, np.float64)
        if nf <= 3:  # not filtered: the constant column is NaN itself
            assert np.isnan(ref[:, col]).all() and np.isnan(got[b, :nr, col]).all()
        else:  # one NaN in a window sorts last: the middle stays finite
            assert np.isfinite(ref[:, col]).all() and np.isfinite(got[b, :nr, col]).all()
        if nf >= 20:  # four in a window of seven: NaN where the window holds all four
            assert np.isnan(ref[:, col + 50: col + 54]).all() and np.isnan(got[b, :nr, col + 50: col + 54]).all()


def test_align_cost_widths():
    n_rows, n_frames = [3, 5, 2], [4, 7, 1500]
    p = _probs(np.random.default_rng(5), 3, 5, 4, 1500)
    for width in (1, 3, 7, 15):
        _check_align_cost(p, n_rows, n_frames, width, f"width {width}")
    lib = _lib.load()
    probs = torch.from_numpy(p).to(DEV)
    cost = torch.full((3, 5, 1500), float("nan"), device=DEV)
    nr = torch.tensor(n_rows, dtype=torch.int32, device=DEV)
    nf = torch.tensor(n_frames, dtype=torch.int32, device=DEV)
    for width in (0, 2, 6, 17, -1):
        assert lib.tw_align_cost(probs.data_ptr(), 3, 5, 4, 1500, nr.data_ptr(), nf.data_ptr(), width,
                                 cost.data_ptr(), S()) != 0, width
    assert lib.tw_align_cost(None, 3, 5, 4, 1500, nr.data_ptr(), nf.data_ptr(), 7, cost.data_ptr(), S()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(cost).all()


# ---------------------------------------------------------------- force_pass on test-mini
CLIPS = [speech_like(30.0, 1234), white_noise(12.3, 7), speech_like(40.0, 5)[: 20 * 16000]]
NF = [-(-len(c) // 160) for c in CLIPS]


def _load(eng, order):
    host = np.zeros((len(order), 480000), np.float32)
    for j, i in enumerate(order):
        host[j, : len(CLIPS[i])] = CLIPS[i]
    eng.wave[: len(order)].copy_(torch.from_numpy(host))
    eng.logmel(len(order))
    eng.encode(len(order), row_map=False, seek=False)


@pytest.fixture(scope="module")
def tr():
    t = TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3)
    t.engine.gen.alignment_heads = list(HEADS)
    yield t
    t.close()


@pytest.fixture(scope="module")
def oracle():
    sd = wo.synth_state_dict(D.d_model, D.encoder_layers, D.decoder_layers, D.ffn, D.n_mels, D.vocab, 1234)
    return wo.WhisperOracle(sd, D.heads)


@pytest.fixture(scope="module")
def encs(oracle):
    return [oracle.encode(wo.log_mel(c, D.n_mels)) for c in CLIPS]


@pytest.fixture(scope="module")
def greedy(tr):
    """Each window's own greedy text tokens (timestamp and special tokens stripped)."""
    eng = tr.engine
    host = np.zeros((3, 480000), np.float32)
    for i, c in enumerate(CLIPS):
        host[i, : len(c)] = c
    eng.wave[:3].copy_(torch.from_numpy(host))
    eng.logmel(3)
    segs = eng.generate(3, task="transcribe", max_new_tokens=40)
    eot = eng.gen.special.eot
    toks = [[t for t in s if t < eot] for s in segs]
    assert all(len(t) >= 3 for t in toks)
    return toks


class _Refs:
    """forced_reference per (window, forced ids), computed once and shared."""

    def __init__(self, oracle, encs, gen):
        self.oracle, self.encs, self.st, self.cache = oracle, encs, gen.special, {}
        g = wo.GenCfg(D.vocab, self.st.eot, self.st.sot, self.st.lang_begin, self.st.n_languages,
                      self.st.transcribe, self.st.translate, self.st.notimestamps, gen.suppress_tokens,
                      gen.begin_suppress_tokens)
        self.langs = [wo.detect_language(oracle, e, g) for e in encs]

    def __call__(self, i, ids):
        key = (i, tuple(ids))
        if key not in self.cache:
            st = self.st
            prompt = [st.sot, self.langs[i], st.transcribe, st.notimestamps]
            self.cache[key] = ar.forced_reference(self.oracle, self.encs[i], prompt, ids, st.eot, HEADS, NF[i])
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(tr, oracle, encs):
    return _Refs(oracle, encs, tr.engine.gen)


def _close_times(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    d = np.abs(got - ref)
    print(f"{what}: {got.size} times, max |d| {d.max():.3f} s, {(d < 1e-6).mean():.0%} equal")
    assert d.max() <= 0.2 + 1e-6, (what, float(d.max()))
    assert (d < 1e-6).mean() >= 0.9, (what, float((d < 1e-6).mean()))


def _close_lps(got, ref, per_token, mean, what):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    dm = abs(float(np.mean(got)) - float(np.mean(ref)))
    print(f"{what}: {d.size} log-probabilities, max |d| {d.max():.4g}, |mean d| {dm:.4g}")
    assert d.max() <= per_token and dm <= mean, (what, float(d.max()), dm)


def _check_pass(eng, refs, order, forced, per_token, mean, what):
    _load(eng, order)
    tail = eng.prompt_tail("transcribe", False)
    res = eng.force_pass(len(order), tail, None, forced, num_frames=[NF[i] for i in order])
    P = eng._prompt_len(tail)
    assert res.lang_ids == [refs.langs[i] for i in order], what
    for j, i in enumerate(order):
        toks, lps, ts = refs(i, forced[j])
        assert res.tokens[j] == toks, (what, j)                      # echoed exactly, <|endoftext|> appended
        assert len(res.token_lp[j]) == len(toks) and len(res.token_ts[j]) == P + len(toks)
        assert not np.asarray(res.token_ts[j][:P]).any()
        _close_lps(res.token_lp[j], lps, per_token, mean, f"{what} row {j}")
        _close_times(res.token_ts[j], ts, f"{what} row {j}")
    return res


def test_force_pass_vs_oracle(tr, refs, greedy):
    eng = tr.engine
    _check_pass(eng, refs, [0, 1, 2], greedy, 0.30, 0.03, "bf16 full")
    # one row forced with a single token (host path), one cut to two (the smallest the kernel standardises)
    _check_pass(eng, refs, [0, 1, 2], [greedy[0][:1], greedy[1][:2], greedy[2]], 0.30, 0.03, "bf16 short")


def test_force_pass_is_independent_of_the_batch(tr, refs, greedy):
    eng = tr.engine
    alone = _check_pass(eng, refs, [0], [greedy[0]], 0.30, 0.03, "alone")
    batch = _check_pass(eng, refs, [1, 0, 2], [greedy[1][:2], greedy[0], greedy[2]], 0.30, 0.03, "as row 1")
    _close_times(batch.token_ts[1], alone.token_ts[0], "row 1 of three vs alone")
    _close_lps(batch.token_lp[1], alone.token_lp[0], 0.30, 0.03, "row 1 of three vs alone")


def test_force_pass_fp32_engine(refs, greedy):
    with TurboTranscriber.from_pretrained("test-mini", seed=1234, max_batch=3, precision="fp32") as t:
        t.engine.gen.alignment_heads = list(HEADS)
        _check_pass(t.engine, refs, [0, 1, 2], [greedy[0], greedy[1][:2], greedy[2][:1]], 1e-3, 1e-3, "fp32")


def test_force_pass_limits(tr, greedy):
    eng = tr.engine
    tail = eng.prompt_tail("transcribe", False)
    limit = eng.max_new_for(eng._prompt_len(tail))
    with pytest.raises(ValueError, match="more than"):
        eng.force_pass(1, tail, None, [[400] * limit])
    with pytest.raises(ValueError, match="vocabulary"):
        eng.force_pass(1, tail, None, [[D.vocab]])
    with pytest.raises(ValueError):
        eng.force_pass(2, tail, None, [[400]])


def test_force_pass_queues_without_host_sync(tr, greedy, monkeypatch):
    """With graphs, a forced pass is the prompt graph and max(len) - 1 replays of one captured step: between the
    first and the last replay the host neither synchronises nor reads a device value, and no step hook runs. The
    graphs survive across calls (the second call captures nothing)."""
    eng = tr.engine
    assert eng.use_graphs
    forced = [greedy[0], greedy[1][:2], greedy[2]]
    _load(eng, [0, 1, 2])
    tail = eng.prompt_tail("transcribe", False)
    nf = [NF[i] for i in range(3)]
    first = eng.force_pass(3, tail, None, forced, num_frames=nf)  # captures
    n_graphs = len(eng._graphs)
    log = []

    def spy(owner, name, tag):
        real = getattr(owner, name)

        def wrapper(*a, **k):
            log.append(tag)
            return real(*a, **k)

        monkeypatch.setattr(owner, name, wrapper)

    spy(torch.cuda, "synchronize", "sync")
    spy(torch.cuda.Stream, "synchronize", "sync")
    spy(torch.cuda.Event, "synchronize", "sync")
    spy(torch.Tensor, "item", "read")
    spy(torch.Tensor, "tolist", "read")
    spy(torch.Tensor, "cpu", "read")
    real_replay = torch.cuda.CUDAGraph.replay

    def replay(self):
        assert eng.step_hook is None
        log.append("replay")
        return real_replay(self)

    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", replay)
    second = eng.force_pass(3, tail, None, forced, num_frames=nf)
    monkeypatch.undo()
    assert len(eng._graphs) == n_graphs
    i0, i1 = log.index("replay"), len(log) - 1 - log[::-1].index("replay")
    assert log[i0: i1 + 1] == ["replay"] * max(len(f) + 1 for f in forced), log
    assert "read" in log[i1:]  # (the spies do see the result being fetched afterwards)
    assert second.tokens == first.tokens
    for a, b in zip(second.token_lp, first.token_lp):
        assert np.allclose(a, b, rtol=0, atol=1e-4)
    for j, (a, b) in enumerate(zip(second.token_ts, first.token_ts)):
        _close_times(a, b, f"second call row {j}")


# ---------------------------------------------------------------- TurboTranscriber.align end to end
def _token_chunks(tr, x):
    """The transcript's chunks as (t0, t1, text token ids), rebuilt from the windows' raw passes (one pass per
    window): the text between two timestamp tokens, at the window's offset."""
    from twamd.frontend import chunk_windows

    st, sr, total = tr.gen.special, tr.sampling_rate, len(x) / tr.sampling_rate
    out = []
    for w, passes in zip(chunk_windows(len(x), 30, None, sr), tr.last_window_passes):
        base, end = w.start / sr, min(total, (w.start + w.length) / sr)
        t0, cur = 0.0, []
        for t in list(passes[0]) + [None]:
            if t is not None and t < st.eot:
                cur.append(int(t))
            elif t is None or t >= st.timestamp_begin:
                t1 = 30.0 if t is None else (t - st.timestamp_begin) * 0.02
                a, b = base + t0, min(end, base + t1)
                if cur and b - a > 0.1:
                    out.append({"timestamp": (round(a, 2), round(b, 2)), "tokens": cur})
                t0, cur = t1, []
    return out


def test_align_end_to_end(tr, oracle):
    x = np.concatenate([speech_like(40.0, 5), white_noise(35.0, 11)])
    r = tr(x, chunk_length_s=30, return_timestamps=True,
           generate_kwargs={"task": "transcribe", "num_beams": 1, "max_new_tokens": 40, "max_passes": 1})
    assert r["chunks"]
    chunks = _token_chunks(tr, x)
    assert len(chunks) >= 2
    chunks.insert(1, {"timestamp": (1.0, 2.0), "tokens": []})      # no tokens: not run, no words
    if len(x) / 16000 - chunks[-1]["timestamp"][0] <= 30.0:
        chunks[-1]["timestamp"] = (chunks[-1]["timestamp"][0], None)   # None: the end of the input
    out = tr.align(x, chunks, language="english", task="transcribe", batch_size=2, return_language=True)
    vocab, st = tr.vocab, tr.gen.special
    assert out["text"] == "".join(vocab.decode(c["tokens"]) for c in chunks)
    assert "".join(w["text"] for w in out["chunks"]) == out["text"]
    assert len(out["chunk_avg_logprob"]) == len(chunks) and out["chunk_avg_logprob"][1] is None
    words = iter(out["chunks"])
    total = len(x) / 16000
    prompt = [st.sot, st.lang_to_id()["<|en|>"], st.transcribe, st.notimestamps]
    for c, avg in zip(chunks, out["chunk_avg_logprob"]):
        if not c["tokens"]:
            continue
        t0, t1 = c["timestamp"][0], total if c["timestamp"][1] is None else c["timestamp"][1]
        n = len(collate_word_timestamps(vocab, list(c["tokens"]), [(0.0, 0.0)] * len(c["tokens"]), "english", False))
        mine = [next(words) for _ in range(n)]
        assert "".join(w["text"] for w in mine) == vocab.decode(c["tokens"])
        flat = [t for w in mine for t in w["timestamp"]]
        assert all(t0 - 0.02 <= t <= t1 + 0.02 for t in flat), (c["timestamp"], flat)
        assert all(a <= b for a, b in zip(flat, flat[1:])), flat
        assert all(0.0 < w["probability"] <= 1.0 and w["language"] == "english" for w in mine)
        seg = x[int(round(t0 * 16000)): int(round(t1 * 16000))]
        _, lps, _ = ar.forced_reference(oracle, oracle.encode(wo.log_mel(seg, D.n_mels)), prompt, c["tokens"],
                                        st.eot, HEADS, -(-len(seg) // 160))
        print(f"align chunk {c['timestamp']}: avg_logprob {avg:.4f}, reference {np.mean(lps[:-1]):.4f}")
        assert abs(avg - float(np.mean(lps[:-1]))) <= 0.03, (c["timestamp"], avg, float(np.mean(lps[:-1])))
    assert next(words, None) is None
