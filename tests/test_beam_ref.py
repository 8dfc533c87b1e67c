"""The host side of tests/test_gpu_beam_lockstep.py, checked without a GPU: oracle.whisper_oracle.beam_search_core's
per-step trace (on_step) changes nothing and ends on the returned trace; the references of tests/beam_ref.py for what
the oracle does not track are self-consistent (the K/V position table gathers each beam's history, the log-probability
terms sum to the sums); and the lockstep cases' inputs meet the precondition and reach the processors' states."""
import numpy as np
import pytest

import beam_ref as br

SMALL = [br.case(n) for n in ("nb2", "nb3", "nb6-nots", "nb5-ties", "nb8-maxnew", "nb3-wide")]


@pytest.mark.parametrize("c", SMALL, ids=repr)
def test_traced_equals_untraced_and_ends_on_the_returned_trace(c):
    for w in range(c.W):
        f = br.window_facts(c, w)
        ref, tr, recs, _ = br.oracle_window(c, w, traced=False)
        assert recs == [] and ref == f["ref"] and tr["steps"] == f["trace"]["steps"] == f["steps"]
        last = f["recs"][-1]
        for a, b in ((tr, f["trace"]), (tr, last)):  # untraced = traced; the last record = the returned trace
            assert a["fin_seq"] == b["fin_seq"] and a["run_tok"] == b["run_tok"] and a["steps"] == b["steps"]
            for k in ("fin_score", "run_score", "fin_flag"):
                assert np.array_equal(a[k], b[k]), k
        assert ref == last["fin_seq"][0]
        assert bool(not last["unsatisfied"] or last["all_hits"])  # the step the core stopped at
        for rec in f["recs"][:-1]:
            assert rec["unsatisfied"] and not rec["all_hits"]
        for t, rec in enumerate(f["recs"]):  # the record's own consistency: the K continuations, ordered
            K = 2 * c.nb
            assert rec["steps"] == t + 1 and len(rec["src"]) == len(rec["tok"]) == len(rec["sc"]) == K
            assert np.all(np.diff(rec["sc"]) <= 0) and np.array_equal(rec["near_val"][:K], rec["sc"])
            assert [rec["prev_run_tok"][s] + [int(x)] for s, x in zip(rec["src"][rec["order"]], rec["tok"][rec["order"]])] \
                == rec["run_tok"]


@pytest.mark.parametrize("c", [br.case("nb3"), br.case("nb5-ties"), br.case("nb8-T5")], ids=repr)
def test_position_table_gathers_each_history_and_terms_sum(c):
    """kv_tab / fin_tab reference: a physical array "row r wrote token x at position q" that the test fills as the
    decoder would (each row writes the token it is fed at its own position); gathering a running beam's fed tokens
    through its table reproduces its history, and a finished slot's through fin_tab its hypothesis. The term
    histories sum to run_lp / fin_lp."""
    L = br.layout(c.lay)
    nb, T = c.nb, c.T
    for w in range(c.W):
        f = br.window_facts(c, w)
        ref = br.WindowRef(c, w, L)
        phys = np.full((c.W * nb, T + br.P + 1), -1, np.int64)  # [device row][position] = token fed there
        for t, rec in enumerate(f["recs"]):
            p = int(ref.pos[0])
            prev_ids = ref.ids.copy()
            if t > 0:  # the step's rows feed the tokens the previous step chose, at position p
                phys[w * nb:(w + 1) * nb, p] = prev_ids
            ref.apply(rec, f["fed"][t])
            assert np.all(ref.pos == br.P + t + 1) and ref.win[2] == t + 1
            for j in range(nb):
                if ref.run_score[j] <= -1e8:
                    continue
                # positions P + 1 .. p hold the history's tokens 0 .. t - 1 (token t is fed by the next step)
                q = np.arange(br.P + 1, min(p + 1, T))
                assert phys[ref.kv_tab[j, q], q].tolist() == rec["run_tok"][j][:len(q)], (t, j)
                assert np.all(ref.kv_tab[j, min(p + 1, T):] == w * nb + j)  # later entries stay the row's own
                assert abs(np.sum(ref.run_tlp[j, :t + 1]) - ref.run_lp[j]) <= 1e-9 * (t + 1)
                assert np.all(np.isnan(ref.run_tlp[j, t + 1:]))
            for s in range(nb):
                n = int(ref.fin_len[s])
                if not ref.fin_flag[s]:
                    assert n == 0 and ref.fin_lp[s] == 0
                    continue
                q = np.arange(br.P + 1, min(br.P + n, T))
                assert phys[ref.fin_tab[s, q], q].tolist() == ref.fin_seq[s][:len(q)], (t, s)
                assert abs(np.sum(ref.fin_tlp[s, :n]) - ref.fin_lp[s]) <= 1e-9 * n
                assert np.all(np.isfinite(ref.fin_tlp[s, :n]))
            # the state rows restate the histories
            for j in range(nb):
                h = rec["run_tok"][j]
                tss = [x for x in h if c.use_ts and x >= L.ts_begin]
                assert ref.state[j, :5].tolist() == [t + 1, h[-1], h[-2] if t else -1, tss[-1] if tss else -1, 0]
                assert ref.src_rows[j] == w * nb + rec["srcs"][j] and ref.ids[j] == h[-1]


@pytest.mark.parametrize("c", br.CASES, ids=repr)
def test_cases_meet_the_precondition(c):
    """Every selection of every step of the case's oracle runs is decided by at least ten times the comparison
    tolerance (beam_ref.check_gaps), the smallest relative gap is the one noted beside the case, the windows finish at
    different steps (a done window keeps being stepped), and a tie case has ties in every row, one straddling the
    K-th place and one between a text and a timestamp token."""
    facts = [br.window_facts(c, w) for w in range(c.W)]
    steps = [f["steps"] for f in facts]
    assert all(s <= c.max_new for s in steps)
    if c.max_new <= 5:
        assert steps == [c.max_new] * c.W and all(f["recs"][-1]["all_hits"] for f in facts)
    elif c.W > 1:
        assert len(set(steps)) > 1, steps
    if c.quant:
        assert {"pair", "straddle", "text_ts"} <= set().union(*[f["ties"] for f in facts])
    assert min(f["gap"] for f in facts) >= 1


def test_the_timestamp_cases_reach_every_processor_state():
    seen = set()
    for name in br.TS_COVERAGE_CASES:
        c = br.case(name)
        for w in range(c.W):
            seen |= br.window_facts(c, w)["coverage"]
    assert seen == set(br.STATES), sorted(set(br.STATES) - seen)
