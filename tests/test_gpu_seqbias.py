"""tw_logits_history_bias on the GPU: the sequence-bias and bad-words stages around the repetition penalty and the
n-gram ban, against the numpy restatement (tests/seqbias_ref.py, pinned to transformers' processors by
tests/test_seqbias_processors.py) — bit for bit on raw logits (the -inf set included), 1e-4 on log-probabilities (as
tests/test_gpu_history.py: another logsumexp order). Rows and tables are test_seqbias_processors' (R = 6, test-mini's
vocabulary, ld = V + 3)."""
import ctypes

import numpy as np
import pytest
import torch

import seqbias_ref as sr
from test_seqbias_processors import (CHAINS, LANG, LONG, POST_ENTRIES, PRE, row_history, seqbias_logits, seqbias_rows)
from twamd import _lib
from twamd.config import PRESETS

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, T = PRESETS["test-mini"].vocab, 448
LD = V + 3


def S():
    return torch.cuda.current_stream().cuda_stream


def _device_rows(rows, finished=None):
    """prefix [R][T], prefix_len, tokens [R][T], state; a row's language slot holds TW_HIST_LANG in the prefix and
    its id in state[TW_ST_LANG]. The slot's id must be LONG[1] for the rows of seqbias_rows()."""
    R = len(rows)
    prefix = np.full((R, T), -7, np.int32)  # (entries past a row's length are never read: any value)
    tokens = np.full((R, T), -7, np.int32)
    plen = np.zeros(R, np.int32)
    state = torch.zeros(R, _lib.TW_STATE_STRIDE, dtype=torch.int32, device=DEV)
    state[:, _lib.TW_ST_LAST:_lib.TW_ST_LASTTS + 1] = -1
    for r, (pre, gen, slot) in enumerate(rows):
        prefix[r, : len(pre)] = pre
        tokens[r, : len(gen)] = gen
        plen[r] = len(pre)
        state[r, _lib.TW_ST_NGEN] = len(gen)
        state[r, _lib.TW_ST_FINISHED] = int(r == finished)
        state[r, _lib.TW_ST_LANG] = LANG
        if slot is not None:
            state[r, _lib.TW_ST_LANG] = pre[slot]
            prefix[r, slot] = _lib.TW_HIST_LANG
    return torch.from_numpy(prefix).to(DEV), torch.from_numpy(plen).to(DEV), torch.from_numpy(tokens).to(DEV), state


class Table:
    """The device arrays of a TwSeqBias for pre + post entries (ids rows of TW_SEQBIAS_MAX_IDS, unused slots -9)."""

    def __init__(self, pre, post, ld=_lib.TW_SEQBIAS_MAX_IDS):
        ent = list(pre) + list(post)
        n = max(len(ent), 1)
        ids = np.full((n, ld), -9, np.int32)
        for e, (seq, _) in enumerate(ent):
            ids[e, : len(seq)] = seq
        self.ids = torch.from_numpy(ids).to(DEV)
        self.len = torch.tensor([len(seq) for seq, _ in ent] or [0], dtype=torch.int32, device=DEV)
        self.bias = torch.tensor([b for _, b in ent] or [0.0], dtype=torch.float32, device=DEV)
        self.n_pre, self.n_post = len(pre), len(post)
        self.struct = _lib.TwSeqBias(self.ids.data_ptr(), self.len.data_ptr(), self.bias.data_ptr(), ld, self.n_pre,
                                     self.n_post)


def _run(lg, R, ld, prefix, plen, tokens, state, p, n, to_lp, table):
    _lib.call("tw_logits_history_bias", lg.data_ptr(), R, ld, V, _lib.ptr(prefix), T if prefix is not None else 0,
              _lib.ptr(plen), tokens.data_ptr(), T, state.data_ptr(), float(p), int(n), int(to_lp),
              ctypes.byref(table.struct) if table is not None else None, S())


@pytest.fixture(scope="module")
def x():
    return seqbias_logits(6, LD)


def test_the_rows_hold_the_cases():
    """The language slot's id is the one the 16-id entry expects, the entry has the maximum id count and its match
    spans the prefix / generated boundary, and the short rows have the history lengths around the 3-id entries."""
    rows = seqbias_rows()
    assert len(LONG) == _lib.TW_SEQBIAS_MAX_IDS and rows[5][0][rows[5][2]] == LONG[1]
    assert len(rows[5][0]) < 15 < len(row_history(rows[5]))  # the 16-id match spans the prefix / generated boundary
    assert [len(row_history(r)) for r in rows[:5]] == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("tables", ["both", "pre_only", "post_only"])
def test_raw_mode_is_bit_equal_to_the_restatement(x, tables):
    """Every (penalty, n-gram) of CHAINS, all rows live and with row 3 finished: the logits equal the restatement's
    five-stage chain bit for bit, finished rows and the padding columns are untouched, state and tokens are not
    written. pre_only / post_only: n_post = 0 / n_pre = 0 alone."""
    pre = PRE if tables != "post_only" else []
    post = POST_ENTRIES if tables != "pre_only" else []
    table = Table(pre, post)
    rows = seqbias_rows()
    R = len(rows)
    for finished in (None, 3):
        prefix, plen, tokens, state = _device_rows(rows, finished)
        s0, t0 = state.clone(), tokens.clone()
        for p, n in CHAINS:
            lg = torch.from_numpy(x).to(DEV)
            _run(lg, R, LD, prefix, plen, tokens, state, p, n, False, table)
            torch.cuda.synchronize()
            got = lg.cpu().numpy()
            for r, row in enumerate(rows):
                ref = x[r, :V] if r == finished else sr.chain(x[r, :V], row_history(row), pre, p, n, post)
                bad = np.flatnonzero(got[r, :V].view(np.int32) != ref.view(np.int32))
                assert bad.size == 0, (tables, p, n, r, finished, bad[:8], got[r, bad[:8]], ref[bad[:8]])
            assert np.array_equal(got[:, V:].view(np.int32), x[:, V:].view(np.int32))
        assert torch.equal(state, s0) and torch.equal(tokens, t0)


def test_the_cases_act_on_the_device(x):
    """What the table is there for, read off the device output of the (1.3, 2) chain: the sum on id 500 in
    transformers' order, -inf from the pre stage, -inf + 5 stays -inf, the L + 1 entry skipped, the 16-id entry across
    the boundary and the language slot, and bad words on ids the penalty and the n-gram ban also touch."""
    rows = seqbias_rows()
    table = Table(PRE, POST_ENTRIES)
    prefix, plen, tokens, state = _device_rows(rows)
    lg = torch.from_numpy(x).to(DEV)
    _run(lg, 6, LD, prefix, plen, tokens, state, 1.3, 2, False, table)
    got = lg.cpu().numpy()
    f32 = np.float32
    pen = lambda v: v * f32(1.3) if v < 0 else v / f32(1.3)  # noqa: E731
    assert got[0, 500] == x[0, 500] + f32(1.0) and got[1, 500] == x[1, 500] + f32(1.0)  # only the 1-id entry
    assert got[2, 960] == x[2, 960]  # [31 1234 960] is one longer than the history [31 1234]: skipped
    assert got[3, 960] == x[3, 960] + f32(7.0) and got[4, 960] == x[4, 960] + f32(7.0) and got[5, 960] == x[5, 960]
    assert np.isneginf(got[2:5, 500]).all()  # the bad word [1234 500] (2 ids: too long for row 1 only)
    assert np.isneginf(got[:, 7]).all() and np.isneginf(got[1:, 50364]).all() and np.isneginf(got[:, 50365]).all()
    assert got[5, LONG[15]] == x[5, LONG[15]] + f32(2.0) and got[5, 950] == x[5, 950] + f32(-2.5)
    assert got[5, 951] == x[5, 951] and got[0, LONG[15]] == x[0, LONG[15]]
    assert np.isneginf(got[2:5, 9]).all() and got[1, 9] == x[1, 9]  # the bad word [1234 9]
    # the same without the bad words: id 500 of row 3 is x + 1.0 (in order), not x + (1 + 2^-23)
    lg = torch.from_numpy(x).to(DEV)
    _run(lg, 6, LD, prefix, plen, tokens, state, 1.0, 0, False, Table(PRE, []))
    got = lg.cpu().numpy()
    assert got[3, 500] == x[3, 500] + f32(1.0) and got[4, 500] == x[4, 500] + f32(1.0)
    # without bad words, row 3's id 9 is penalised and row 4's is banned by the 2-gram
    lg = torch.from_numpy(x).to(DEV)
    _run(lg, 6, LD, prefix, plen, tokens, state, 1.3, 2, False, Table(PRE, []))
    got = lg.cpu().numpy()
    assert got[3, 9] == pen(x[3, 9]) and np.isneginf(got[4, 9])


@pytest.mark.parametrize("table", ["null", "empty"])
def test_null_table_is_tw_logits_history(x, table):
    rows = seqbias_rows()
    prefix, plen, tokens, state = _device_rows(rows)
    for to_lp in (False, True):
        a, b = torch.from_numpy(x).to(DEV), torch.from_numpy(x).to(DEV)
        _lib.call("tw_logits_history", a.data_ptr(), 6, LD, V, prefix.data_ptr(), T, plen.data_ptr(),
                  tokens.data_ptr(), T, state.data_ptr(), 1.3, 2, int(to_lp), S())
        _run(b, 6, LD, prefix, plen, tokens, state, 1.3, 2, to_lp, None if table == "null" else Table([], []))
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert not torch.equal(a, torch.from_numpy(x).to(DEV))


def test_torch_op_addresses_views_by_their_row_stride(x):
    """torch.ops.tw.logits_history_bias_ on column-sliced views of wider buffers (tokens, prefix, logits[:, :V] of
    ld = V + 3, and the table's ids as the first 16 columns' worth of a view) equals the C-ABI call."""
    from twamd import _ops

    tw = _ops.load()
    rows = seqbias_rows()
    prefix, plen, tokens, state = _device_rows(rows)
    table = Table(PRE, POST_ENTRIES)
    a, b = torch.from_numpy(x).to(DEV), torch.from_numpy(x).to(DEV)
    _run(a, 6, LD, prefix, plen, tokens, state, 1.3, 2, False, table)
    spare = torch.cat([table.ids, table.ids[:3]])  # (more rows than entries)
    tw.logits_history_bias_(b[:, :V], V, prefix[:, :8], plen, tokens[:, :64], state, 1.3, 2, False, spare[:, :12],
                            table.len, table.bias, table.n_pre, table.n_post)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(a, torch.from_numpy(x).to(DEV))


@pytest.mark.parametrize("p,n", CHAINS)
def test_logprob_mode_against_float64(x, p, n):
    """to_logprobs: the -inf set is exact and finite values are within 1e-4 of the float64 restatement (the bound and
    the reason of tests/test_gpu_history.py: scores under 64 in magnitude, an f32 ulp ~4e-6, a tree-summed logsumexp
    over 5e4 terms; the biases add at most one more rounding of that size)."""
    rows = seqbias_rows()
    table = Table(PRE, POST_ENTRIES)
    prefix, plen, tokens, state = _device_rows(rows)
    lg = torch.from_numpy(x).to(DEV)
    _run(lg, 6, LD, prefix, plen, tokens, state, p, n, True, table)
    got = lg.cpu().numpy()
    for r, row in enumerate(rows):
        ref = sr.chain(x[r, :V].astype(np.float64), row_history(row), PRE, p, n, POST_ENTRIES, to_logprobs=True)
        assert np.array_equal(np.isneginf(got[r, :V]), np.isneginf(ref)), r
        fin = np.isfinite(ref)
        err = np.abs(got[r, :V][fin] - ref[fin]).max()
        print(f"p={p} n={n} row {r}: max |err| {err:.2e}")
        assert err <= 1e-4, (r, err)
    assert np.array_equal(got[:, V:].view(np.int32), x[:, V:].view(np.int32))
