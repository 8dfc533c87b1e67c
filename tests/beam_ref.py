"""Host reference of everything tw_beam_step writes, step by step, from oracle.whisper_oracle.beam_search_core's
per-step trace (on_step): the oracle tracks the hypotheses and their scores; this module adds, in plain numpy, what
it does not — the processor state rows, src_rows / ids / pos / win, the copy-free K/V position table (kv_tab) and the
finished hypotheses' tables (fin_tab), and the renormalised log-probability sums and terms (run_lp / fin_lp /
run_tlp / fin_tlp). It also holds the lockstep cases (inputs chosen on the CPU, tests/test_beam_ref.py), the
precondition that makes a lockstep comparison meaningful (check_gaps) and the processor-state coverage count."""
import numpy as np

import confidence_ref as cr
import history_ref as hr
from oracle import whisper_oracle as wo

ST_NGEN, ST_LAST, ST_PENULT, ST_LASTTS, ST_FINISHED = 0, 1, 2, 3, 4  # include/tw_whisper.h
STATE_STRIDE = 8
P = 3  # prompt length of every case (pos starts there)
TOK_SENTINEL = -77  # tokens / fin_tokens / fin_tab / state words 5..7 / win[3] before a pass
NEG = np.float32(-1e9)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def synthetic_logits(history, V, tsb, eot, salt, quant=0.0, hot=(), _cache={}):
    """Deterministic logits of a beam's token history and the window's salt (the generator of tests/test_gpu_beam.py:
    seeded Gaussian, a few boosted text and timestamp tokens, an EOS that grows likelier with length), memoised so
    that the oracle and the device loop share one array per history. The timestamp boosts sit within 60 of the last
    timestamp of the history so that passes walk through text-timestamp-timestamp-text (every mask of the Whisper
    processors), and every boost is drawn from a range of several units so that the candidates' scores lie apart.
    quant > 0 rounds to its multiples (exact ties). hot: ids boosted at every step, so that beams repeat ids and
    2-grams (the history processors' cases). A vocabulary without timestamps (tsb >= V) gets no timestamp boosts."""
    key = (V, tsb, salt, quant) + ((tuple(hot),) if hot else ()) + tuple(int(t) for t in history)
    if key not in _cache:
        rng = np.random.default_rng(hash(key) & 0xFFFFFFFF)
        x = rng.standard_normal(V).astype(np.float32) * 1.5
        x[rng.integers(0, min(tsb, V), 8)] += rng.uniform(5.0, 13.0, 8).astype(np.float32)
        if tsb + 60 <= V:
            tss = [t for t in history if t >= tsb]
            base = min(tss[-1], V - 61) if tss else tsb
            x[base + rng.integers(0, 60, 5)] += rng.uniform(5.0, 12.0, 5).astype(np.float32)
        x[eot] += 5.0 + 0.5 * len(history)
        x[list(hot)] += 9.0
        if quant:
            x = (np.round(x / np.float32(quant)) * np.float32(quant)).astype(np.float32)
        _cache[key] = x
    return _cache[key]


class Layout:
    """The token layout a case runs on: the fields of GenCfg / TwSelectParams."""

    def __init__(self, name, V, eot, sot, lang_begin, n_lang, transcribe, translate, notimestamps, suppress,
                 begin_suppress, mit=50):
        self.name, self.V, self.eot, self.sot, self.lang_begin, self.n_lang = name, V, eot, sot, lang_begin, n_lang
        self.transcribe, self.translate, self.notimestamps = transcribe, translate, notimestamps
        self.ts_begin = notimestamps + 1
        self.suppress, self.begin_suppress, self.mit = list(suppress), list(begin_suppress), mit

    def gcfg(self, null_mask=False):
        return wo.GenCfg(self.V, self.eot, self.sot, self.lang_begin, self.n_lang, self.transcribe, self.translate,
                         self.notimestamps, [] if null_mask else self.suppress, self.begin_suppress, self.mit)


def layout(name):
    """"test-mini" (51866) and "tiny.en" (51864, other ts_begin) from the package's presets; "wide": a made-up 70001
    vocabulary without timestamp tokens, whose 16 chunks hold 4375 > 16 * 256 tokens each."""
    if name == "wide":
        return Layout(name, 70001, 50257, 50258, 50259, 100, 50359, 50358, 70000,
                      [1, 2, 7, 8, 9, 10, 14, 25, 50258, 50358, 50359, 50360, 50361, 50362, 60000, 69999, 70000],
                      [220, 50257])
    from twamd.config import PRESETS, GenerationSettings
    d = PRESETS[name]
    gen = GenerationSettings.default(d)
    st = gen.special
    return Layout(name, d.vocab, st.eot, st.sot, st.lang_begin, st.n_languages, st.transcribe, st.translate,
                  st.notimestamps, gen.suppress_tokens, gen.begin_suppress_tokens, gen.max_initial_timestamp_index)


class Case:
    """One lockstep pass: W windows x nb beams. salts: one per window. opt: the
    optional outputs given (kv_tab, fin_tab, run_lp, fin_lp, run_tlp, fin_tlp) or all NULL. ld_pad: ld_logits - V.
    hist: (repetition_penalty, no_repeat_ngram_size) of a tw_logits_history(to_logprobs) pass ahead of every step
    (scores_are_logprobs = 1), else None."""

    def __init__(self, name, nb, salts, use_ts=True, max_new=24, T=448, opt=True, lay="test-mini", ld_pad=0,
                 null_mask=False, lp=1.0, quant=0.0, hist=None):
        self.name, self.nb, self.salts, self.W, self.use_ts = name, nb, tuple(salts), len(salts), use_ts
        self.max_new, self.T = max_new, T
        self.opt, self.lay, self.ld_pad, self.null_mask, self.lp, self.quant, self.hist = (opt, lay, ld_pad, null_mask,
                                                                                          lp, quant, hist)

    def __repr__(self):
        return self.name

    @property
    def hot(self):
        return (1000, 2000, 3000) if self.hist else ()

    def prefix(self, w, L):
        """The prompt ids the history processors of window w see (hist cases)."""
        return [2000 + w, 3000, L.sot, L.lang_begin + w, L.transcribe][-(3 + 2 * (w % 2)):]


# The salts were picked on the CPU by running the oracle alone (a loop over window_facts; tests/test_beam_ref.py::
# test_cases_meet_the_precondition re-checks them): per window the first salts at which every step meets check_gaps,
# the windows of a case finish at different steps and a tie case meets every kind of tie. The trailing comment is the
# smallest relative gap of the case (gap / (1e-3 + 1e-4 |score|), so >= 1).
CASES = [
    # every width, timestamps on, every optional output
    Case("nb2", 2, (0, 1)),  # 7.84
    Case("nb3", 3, (2, 3)),  # 1.36
    Case("nb4", 4, (5, 10)),  # 1.21
    Case("nb5", 5, (3, 11)),  # 1.07
    Case("nb6", 6, (13, 15)),  # 1.08
    Case("nb7", 7, (15, 128)),  # 1.01
    Case("nb8", 8, (82, 1109)),  # 1.09
    # every optional pointer NULL
    Case("nb8-null", 8, (82, 1109), opt=False),  # 1.09
    Case("nb4-null", 4, (5, 10), opt=False),  # 1.21
    # no timestamps
    Case("nb8-nots", 8, (1808, 1834), use_ts=False),  # 1.17
    Case("nb7-nots", 7, (129, 143), use_ts=False),  # 1.03
    Case("nb6-nots", 6, (5, 27), use_ts=False),  # 1.05
    # the row index arithmetic w * nb + j
    Case("nb8-W1", 8, (82,)),  # 1.09
    Case("nb8-W3", 8, (82, 1109, 1142)),  # 1.09
    # exact ties: logits in multiples of 0.5
    Case("nb5-ties", 5, (0, 19), quant=0.5),  # 2.06
    Case("nb8-ties", 8, (44, 157), quant=0.5),  # 1.16
    # a row stride past V (NaN pad) and no suppress mask
    Case("nb8-stride-nullmask", 8, (82, 1109), ld_pad=37, null_mask=True),  # 1.09
    # other layouts
    Case("nb5-tiny.en", 5, (1, 28), lay="tiny.en"),  # 1.38
    Case("nb8-logprobs", 8, (825, 855), hist=(1.3, 2)),  # 1.01
    Case("nb8-lp0.5", 8, (82, 120), lp=0.5),  # 1.22
    Case("nb8-lp-2", 8, (5, 62), lp=-2.0),  # 1.22
    Case("nb8-T5", 8, (0, 2), max_new=5, T=5),  # 1.42
    # the tail loop of k_beam_partial (a chunk of more than 4096 tokens)
    Case("nb3-wide", 3, (0, 1), use_ts=False, lay="wide", max_new=16),  # 2.54
    # every window ends by max_new with all candidates hit: the just-finished top-nb fill the slots
    Case("nb8-maxnew", 8, (0, 2), max_new=3),  # 2.40
]
TS_COVERAGE_CASES = [c.name for c in CASES if c.use_ts and c.lay == "test-mini" and not c.hist]


def case(name):
    return next(c for c in CASES if c.name == name)


# ---- the oracle side of a case --------------------------------------------------------------------------------------
class patched_processors:
    """For a hist case: oracle.whisper_oracle's processor chain with the history processors (tests/history_ref.py) in
    front, as tw_logits_history(to_logprobs) puts them in front of tw_beam_step (the pattern of
    tests/test_gpu_history.py::test_beam_step_after_the_history_pass)."""

    def __init__(self, c, w, L):
        self.c, self.pre = c, (c.prefix(w, L) if c.hist else None)

    def __enter__(self):
        if self.c.hist:
            self.orig = orig = wo.process_logits_no_rule
            pen, n, pre = self.c.hist[0], self.c.hist[1], self.pre
            wo.process_logits_no_rule = lambda s, sampled, g: orig(
                hr.history_processors(s, pre + [int(t) for t in sampled], pen, n), sampled, g)
        return self

    def __exit__(self, *a):
        if self.c.hist:
            wo.process_logits_no_rule = self.orig


def oracle_window(c, w, traced=True):
    """beam_search_core on window w of case c. Returns (best hypothesis, final trace, per-step records, fed) with
    fed[t][b] the logits the step-t row of beam b was given."""
    L = layout(c.lay)
    g = L.gcfg(c.null_mask)
    args = (L.V, L.ts_begin, L.eot, c.salts[w], c.quant, c.hot)
    first = synthetic_logits([], *args)
    h = {"h": [[] for _ in range(c.nb)]}
    fed = [[first] * c.nb]

    def step(srcs, toks):
        h["h"] = [h["h"][s] + [int(t)] for s, t in zip(srcs, toks)]
        fed.append([synthetic_logits(x, *args) for x in h["h"]])
        return fed[-1]

    recs = []
    with patched_processors(c, w, L):
        ref, tr = wo.beam_search_core(first, step, P, c.max_new, g, c.use_ts, c.nb, c.lp,
                                      **({"on_step": recs.append} if traced else {}))
    return ref, tr, recs, fed


# ---- the precondition -----------------------------------------------------------------------------------------------
def _tol(v):
    """Ten times the project's rule for these sums (rtol 1e-5, atol 1e-4)."""
    return 1e-3 + 1e-4 * abs(float(v))


def check_gaps(rec, nb, V):
    """The kernel and the oracle sum the log-softmax in different f32 orders, so a selection decided by less than that
    difference is not the kernel's to reproduce. Asserts, on the oracle's record alone, that every selection of the
    step is decided by at least _tol: the top-K (and the K + 1-th it leaves out), the running top-nb, the finished
    top-nb, the timestamp rule and the early-stop comparison. Equal accumulated scores are allowed within one beam
    row only (one logit value, one running score: equal on both sides by construction). Returns the smallest
    gap / _tol seen (>= 1)."""
    K = 2 * nb
    worst = np.inf
    # a. the top-K and its order
    val, idx = rec["near_val"].astype(np.float64), rec["near_idx"]
    assert np.all(np.isfinite(val)), "a masked candidate among the K + 1 best"
    for a in range(K):
        if val[a] == val[a + 1]:
            assert idx[a] // V == idx[a + 1] // V, ("equal scores of two beam rows", a, val[a])
        else:
            r = (val[a] - val[a + 1]) / _tol(val[a])
            assert r >= 1, ("top-K", a, val[a], val[a + 1])
            worst = min(worst, r)
    # e. the running beams: the first nb non-hit continuations in the top-K's order; a hit one (score - 1e9, rounded
    # to a multiple of 64) enters only when there are fewer, and then its rounding must not hang on the last bits
    hits, sc = rec["hits"], rec["sc"].astype(np.float64)
    if int((~hits).sum()) < nb:
        for c in np.nonzero(hits)[0]:
            lo, hi = np.float32(sc[c] - _tol(sc[c]) - 1e9), np.float32(sc[c] + _tol(sc[c]) - 1e9)
            assert lo == hi, ("running beam at -1e9", c, sc[c])
    # f. the finished beams: previous and just-finished real scores (the others sit at <= -1e9, where ties keep the
    # lower, previous, entry and no candidate ever passes a previous one)
    m = np.sort(rec["merged"][rec["merged"] > -1e8].astype(np.float64))[::-1]
    for a in range(len(m) - 1):
        r = (m[a] - m[a + 1]) / _tol(m[a])
        assert r >= 1, ("finished", m[a], m[a + 1])
        worst = min(worst, r)
    # the timestamp rule
    for b in range(nb):
        mg = rec["margin"][b]
        if np.isfinite(mg):
            assert abs(mg) >= 1e-3, ("timestamp rule", b, mg)
            worst = min(worst, abs(mg) / 1e-3)
    # g. the early stop: best running score at this length against the worst finished one
    bp = float(rec["best_possible"])
    for wv in np.atleast_1d(rec["worst"]).astype(np.float64):
        if wv > -1e8 or bp > -1e8:
            r = abs(bp - wv) / _tol(wv if wv > -1e8 else bp)
            assert r >= 1, ("early stop", bp, wv)
            worst = min(worst, r)
    return worst


def row_ties(c, rec, fed_t, L, w=0):
    """For the tie cases: per live beam row of the step, the processed log-probabilities' top K + 1; returns the set
    of {"pair" (equal values inside the row's top K), "straddle" (the K-th equals the K + 1-th), "text_ts" (a text and
    a timestamp token with equal values inside the top K)} for every row (a list of sets)."""
    K = 2 * c.nb
    g = L.gcfg(c.null_mask)
    out = []
    for b in range(c.nb):
        s = wo.process_logits(np.asarray(fed_t[b], np.float32), rec["prev_run_tok"][b], g, c.use_ts)
        top = wo._topk_desc(s, K + 1)
        v = s[top]
        kinds = set()
        for a in range(K):
            if np.isfinite(v[a]) and v[a] == v[a + 1]:
                kinds.add("pair" if a < K - 1 else "straddle")
                if a < K - 1:
                    same = [i for i in top[:K] if s[i] == v[a]]
                    if min(same) < L.ts_begin <= max(same):
                        kinds.add("text_ts")
        out.append(kinds)
    return out


# ---- coverage -------------------------------------------------------------------------------------------------------
STATES = ["initial", "mask_ts_all", "mask_text_lt_eos", "ts_hi_block=last_ts", "ts_hi_block=last_ts+1", "rule_fires",
          "rule_silent", "eos_before_max_new", "src_is_another_beam"]


def coverage(c, recs, L):
    """The processor states (row_mask of csrc/decode.hip) and beam events a traced window met, counted only on rows
    that gave the step a selected continuation (their masks decided an output)."""
    seen = set()
    tb = L.ts_begin
    for rec in recs:
        for b in set(int(x) for x in rec["src"]):
            h = rec["prev_run_tok"][b]
            n = len(h)
            if n == 0:
                seen.add("initial")
                continue
            last_ts, pen_ts = h[-1] >= tb, n < 2 or h[-2] >= tb
            if last_ts and n >= 2 and pen_ts:
                seen.add("mask_ts_all")
            if last_ts and not pen_ts:
                seen.add("mask_text_lt_eos")
            if any(t >= tb for t in h):
                seen.add("ts_hi_block=last_ts" if (last_ts and not pen_ts) else "ts_hi_block=last_ts+1")
            seen.add("rule_fires" if rec["fires"][b] else "rule_silent")
        for i in rec["msel"]:
            if i >= c.nb and rec["tok"][i - c.nb] == L.eot and rec["steps"] < c.max_new:
                seen.add("eos_before_max_new")
        if any(int(s) != j for j, s in enumerate(rec["srcs"]) if rec["run_score"][j] > -1e8):
            seen.add("src_is_another_beam")
    return seen


# ---- what the oracle does not track ---------------------------------------------------------------------------------
class WindowRef:
    """One window's device arrays as tw_beam_step must leave them after every step (rows are the window's own:
    row j here is device row w * nb + j; src_rows and the table entries are device rows). Before the pass the test
    fills the device arrays as reset() does."""

    def __init__(self, c, w, L):
        self.c, self.w, self.L, self.g = c, w, L, L.gcfg(c.null_mask)
        nb, T = c.nb, c.T
        self.t = 0
        self.state = np.full((nb, STATE_STRIDE), TOK_SENTINEL, np.int32)
        self.state[:, ST_NGEN] = 0
        self.state[:, ST_LAST:ST_LASTTS + 1] = -1
        self.state[:, ST_FINISHED] = 0
        self.tokens = np.full((nb, T), TOK_SENTINEL, np.int32)
        self.ids = np.full(nb, TOK_SENTINEL, np.int32)
        self.pos = np.full(nb, P, np.int32)
        self.src_rows = np.full(nb, TOK_SENTINEL, np.int32)
        self.win = np.array([1, 0, 0, TOK_SENTINEL], np.int32)
        self.run_score = np.full(nb, NEG, np.float32)
        self.run_score[0] = 0
        self.fin_score = np.full(nb, NEG, np.float32)
        self.fin_flag = np.zeros(nb, np.int32)
        self.fin_len = np.zeros(nb, np.int32)
        self.fin_seq = [[] for _ in range(nb)]
        self.kv_tab = np.repeat((w * nb + np.arange(nb, dtype=np.int32))[:, None], T, 1)
        self.fin_tab = np.full((nb, T), TOK_SENTINEL, np.int32)
        self.run_lp, self.fin_lp = np.zeros(nb), np.zeros(nb)
        self.run_tlp, self.fin_tlp = np.full((nb, T), np.nan), np.full((nb, T), np.nan)

    def terms(self, rec, fed_t):
        """Each of the K continuations' own log-probability term: x - logsumexp(allowed) of its source row's
        processed scores (the allowed timestamps alone when the rule fires), in float64 (confidence_ref)."""
        out = np.empty(len(rec["tok"]))
        rows = {}
        for k, (b, tok) in enumerate(zip(rec["src"], rec["tok"])):
            b = int(b)
            if b not in rows:
                x = np.asarray(fed_t[b], np.float32)
                lsm = (x.astype(np.float64) - cr.logsumexp(x)).astype(np.float32)  # beam search scores log-probs
                rows[b] = cr.step_logprobs(lsm, rec["prev_run_tok"][b], self.g, self.c.use_ts)
            out[k] = rows[b][int(tok)]
        return out

    def apply(self, rec, fed_t):
        c, nb, T, t, w = self.c, self.c.nb, self.c.T, self.t, self.w
        tb = self.L.ts_begin
        assert rec["steps"] == t + 1
        p = int(self.pos[0])  # the position this step's rows fed
        with patched_processors(c, w, self.L):
            term = self.terms(rec, fed_t)
        src, tok, order, msel = rec["src"], rec["tok"], rec["order"], rec["msel"]
        # finished slots (from the old running arrays, before they move)
        fin_tab, fin_lp, fin_tlp = self.fin_tab.copy(), self.fin_lp.copy(), self.fin_tlp.copy()
        fin_len = self.fin_len.copy()
        for s, i in enumerate(msel):
            if i < nb:  # a kept slot keeps its length, its table (whole row), its sum and its terms
                fin_len[s] = self.fin_len[i]
                fin_tab[s] = self.fin_tab[i]
                fin_lp[s] = self.fin_lp[i]
                fin_tlp[s, :self.fin_len[i]] = self.fin_tlp[i, :self.fin_len[i]]
            else:  # just finished: its source's table over [0, p], 0 beyond; the source's terms and its own
                k = i - nb
                b = int(src[k])
                fin_len[s] = t + 1
                fin_tab[s] = 0
                fin_tab[s, :min(p + 1, T)] = self.kv_tab[b, :min(p + 1, T)]
                fin_lp[s] = self.run_lp[b] + term[k]
                fin_tlp[s, :t] = self.run_tlp[b, :t]
                fin_tlp[s, t] = term[k]
        # running beams
        state, kv_tab, run_lp, run_tlp = self.state.copy(), self.kv_tab.copy(), self.run_lp.copy(), self.run_tlp.copy()
        for j, k in enumerate(order):
            b, x = int(src[k]), int(tok[k])
            assert b == int(rec["srcs"][j]) and x == rec["run_tok"][j][-1]
            state[j, ST_NGEN] = t + 1
            state[j, ST_PENULT] = self.state[b, ST_LAST]
            state[j, ST_LAST] = x
            state[j, ST_LASTTS] = x if (c.use_ts and x >= tb) else self.state[b, ST_LASTTS]
            state[j, ST_FINISHED] = 0
            kv_tab[j, :min(p + 1, T)] = self.kv_tab[b, :min(p + 1, T)]
            run_lp[j] = self.run_lp[b] + term[k]
            run_tlp[j, :t] = self.run_tlp[b, :t]
            run_tlp[j, t] = term[k]
            self.tokens[j, :t + 1] = rec["run_tok"][j]
            self.ids[j] = x
            self.src_rows[j] = w * nb + b
        self.state, self.kv_tab, self.run_lp, self.run_tlp = state, kv_tab, run_lp, run_tlp
        self.fin_tab, self.fin_lp, self.fin_tlp, self.fin_len = fin_tab, fin_lp, fin_tlp, fin_len
        self.pos += 1
        self.run_score = rec["run_score"].copy()
        self.fin_score = rec["fin_score"].copy()
        self.fin_flag = rec["fin_flag"].astype(np.int32)
        self.fin_seq = [list(s) for s in rec["fin_seq"]]
        assert [len(s) for s in self.fin_seq] == list(self.fin_len)
        self.win = np.array([int(rec["unsatisfied"]), int(not rec["unsatisfied"] or rec["all_hits"]), t + 1,
                             TOK_SENTINEL], np.int32)
        self.t = t + 1
        return self


def window_facts(c, w, _cache={}):
    """Window w of case c on the oracle alone: the records, the logits fed, the smallest relative gap of check_gaps
    over the steps (which asserts the precondition), the coverage, and for a tie case the kinds of ties met (asserting
    that every live row of every step has an equal pair among its top 2 * nb)."""
    key = (c.nb, c.salts[w], c.use_ts, c.max_new, c.lay, c.null_mask, c.lp, c.quant, c.hist, w if c.hist else 0)
    if key not in _cache:
        L = layout(c.lay)
        ref, tr, recs, fed = oracle_window(c, w)
        gap, ties = np.inf, set()
        for t, rec in enumerate(recs):
            gap = min(gap, check_gaps(rec, c.nb, L.V))
            if c.quant:
                rt = row_ties(c, rec, fed[t], L)
                for b in range(c.nb):
                    if rec["prev_run_score"][b] > -1e8:
                        assert "pair" in rt[b], ("a row without a tie among its top 2 * nb", t, b)
                        ties |= rt[b]
        if c.hist:  # the history processors must act on continuations that were selected
            pre = c.prefix(w, L)
            assert any(int(x) in pre + rec["prev_run_tok"][int(b)] for rec in recs for b, x in zip(rec["src"], rec["tok"]))
        _cache[key] = {"ref": ref, "trace": tr, "recs": recs, "fed": fed, "gap": gap, "ties": ties,
                       "coverage": coverage(c, recs, L), "steps": len(recs)}
    return _cache[key]
