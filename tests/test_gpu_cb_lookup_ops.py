"""GPU: cb_lookup_step_kernel (csrc/cb_lookup/cb_lookup.hip) through sv_op_cb_lookup_step, one launch on synthetic fp32 logits, against the
Python restatement CbLookupState.step.  The restatement's chooser is the PLAIN step's selection on the same row and state (sv_op_cb_select:
cb_step_kernel itself, held to its own references by tests/test_gpu_vllm_sampling.py), so the comparison says: row j of a slot is selected
exactly as the one-token-per-step batch would select it after the slot's first j tokens of this launch -- and nothing else of the state
moves.  Designed rows check the selection's own rules on top: a tie goes to the lowest id, a sampling slot draws what the sampler op draws
with (seed, column, 0), a row of NaNs emits id 0 and raises `bad`."""
import pytest
import torch

import starvector_amd.engine as E
from starvector_amd import lookup as LK
from tests.gpu_util import dev

pytestmark = pytest.mark.gpu


def _creq(r, base):
    vl = r.get("semantics") == "vllm"
    return LK.CbRequest(budget=r["max_new_tokens"], eos=r.get("eos_token_id", 0), stop=tuple(r.get("stop_ids") or ()),
                        stop_any=tuple(r.get("stop_any_ids") or ()) if vl else (), min_new=r.get("min_new_tokens", 0), base=base)


class _Case:
    """n slots of K + 1 rows over `lg` [n * K1, V]; slot s: request, prompt length, history, live flag and the accepted-run length it is built for"""

    def __init__(self, V, K, seed):
        self.V, self.K, self.K1 = V, K, K + 1
        self.g = torch.Generator().manual_seed(seed)
        self.reqs, self.base, self.hist, self.live, self.run, self.rows_lg = [], [], [], [], [], []

    def slot(self, req, hist, run, base=37, live=1, lg=None):
        rows = 2.0 * torch.randn(self.K1, self.V, generator=self.g) if lg is None else lg
        self.reqs.append(req); self.base.append(base); self.hist.append(list(hist)); self.live.append(live); self.run.append(run)
        self.rows_lg.append(rows)
        return rows

    def select(self, s, j, hist):
        """the plain step's choice on row j of slot s after `hist`; a row without a finite logit has none (an id outside the vocabulary)"""
        if not bool(torch.isfinite(self.rows_lg[s][j]).any()):
            return self.V
        return int(E.op_cb_select(self.rows_lg[s][j:j + 1].to(dev()), [self.reqs[s]], [hist])[0])

    def build(self):
        """the step in flight: run[s] right drafts, then (if room) a wrong one -- the next id of the chain plus one"""
        self.rows, self.pos, self.nd, self.chain = [], [], [], []
        for s in range(len(self.reqs)):
            hist, chain = list(self.hist[s]), []
            for j in range(self.K1):                     # what every row would emit if all drafts in front of it were right
                chain.append(self.select(s, j, hist + chain))
            drafts = chain[:self.run[s]]
            if len(drafts) < self.K:
                drafts.append((chain[len(drafts)] + 1) % self.V)
            last, pos0 = (hist[-1] if hist else 0), self.base[s] + len(hist) - 1
            nd = len(drafts)
            self.rows.append([last] + drafts + [last] * (self.K - nd))
            self.pos.append([pos0] + [pos0 + j for j in range(1, nd + 1)] + [pos0] * (self.K - nd))
            self.nd.append(nd)
            self.chain.append(chain)
        return self

    def restated(self, max_ngram=3, min_ngram=1, forced=None):
        n = len(self.reqs)
        st = LK.CbLookupState(n * self.K1, self.K, max_ngram, min_ngram, vocab=self.V, forced=forced)
        for s in range(n):
            st.req[s], st.live[s], st.hist[s], st.n_draft[s] = _creq(self.reqs[s], self.base[s]), bool(self.live[s]), list(self.hist[s]), self.nd[s]
            st.cur_tok[s * self.K1:(s + 1) * self.K1] = self.rows[s]
            st.positions[s * self.K1:(s + 1) * self.K1] = self.pos[s]
        L0 = [len(h) for h in self.hist]
        st.step(lambda s, col, prefix, hold: self.select(s, col - L0[s], prefix))
        return st

    def launch(self, max_ngram=0, min_ngram=0, forced=None, logprobs=None):
        lg = torch.cat(self.rows_lg, 0).to(dev())
        return E.op_cb_lookup_step(lg, self.K, self.reqs, self.base, self.live, self.hist, self.rows, self.pos, self.nd, max_ngram, min_ngram,
                                   forced=forced, logprobs=logprobs)

    def check(self, out, st):
        n = len(self.reqs)
        assert out["live"] == [int(v) for v in st.live[:n]]
        assert out["history"] == [st.hist[s] for s in range(n)]
        assert out["rows"] == [st.rows_of(s) for s in range(n)] and out["positions"] == [st.positions_of(s) for s in range(n)]
        assert out["n_draft"] == st.n_draft[:n] and out["counts"] == st.counts[:n]
        assert out["finished"] == st.events and out["bad"] == st.bad


def _mixed(V, K, n):
    c = _Case(V, K, seed=7000 + V + 16 * K + n)
    runs = [K, min(1, K), 0, K, 0][:n] if n > 1 else [K]
    hist = [int(x) for x in torch.randint(0, V, (9,), generator=c.g)]
    hist = hist[:4] + hist[:4] + hist[:1]                # a repeat: the lookup behind the step has something to find
    # 0: greedy with a tie in every row -- the two best ids carry the same value
    lg = c.slot(dict(max_new_tokens=60, eos_token_id=-1), hist, runs[0])
    top = lg.topk(2, -1).indices
    for j in range(K + 1):
        lg[j, top[j, 1]] = lg[j, top[j, 0]]
    if n > 1:
        c.slot(dict(max_new_tokens=60, eos_token_id=-1, do_sample=True, temperature=0.9, top_k=50, top_p=0.9, seed=4242), hist[:5], runs[1])
        c.slot(dict(max_new_tokens=60, eos_token_id=-1, repetition_penalty=1.3), hist, runs[2])
        c.slot(dict(semantics="vllm", max_new_tokens=60, eos_token_id=-1, prompt_ids=hist[:2], repetition_penalty=1.2, frequency_penalty=0.5,
                    presence_penalty=0.3, logit_bias={hist[0]: 1.5, (hist[1] + 1) % V: -0.7}), hist[2:], runs[3])
        c.slot(dict(max_new_tokens=60, eos_token_id=-1), hist[:3], runs[4], live=0)          # dead: left untouched
    return c.build(), top


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("K", [1, 3, 15])
@pytest.mark.parametrize("V", [1000, 49157])
def test_one_launch_is_the_restatement(V, K, n):
    c, top = _mixed(V, K, n)
    out = c.launch()
    c.check(out, c.restated())
    # accepted-run lengths as built: K, 1, 0, K -- and the counters say so
    want = [[1, c.nd[s], c.run[s]] for s in range(n)]
    if n == 5:
        want[4] = [0, 0, 0]
        assert out["history"][4] == c.hist[4] and out["rows"][4] == c.rows[4] and out["positions"][4] == c.pos[4] and out["live"][4] == 0
    assert out["counts"] == want
    # the tie: the lower of the two equal best ids, row after row
    L0 = len(c.hist[0])
    assert out["history"][0][L0:] == [int(min(top[j])) for j in range(K + 1)]
    if n == 5:
        # the sampling slot: every emitted token is the sampler op's draw on that row with (seed, column, row 0)
        r, L1 = c.reqs[1], len(c.hist[1])
        emitted = out["history"][1][L1:]
        assert len(emitted) == c.run[1] + 1
        for j, tok in enumerate(emitted):
            draw = E.op_sample_top_p(c.rows_lg[1][j:j + 1].to(dev()), r["temperature"], r["top_p"], r["seed"], L1 + j, top_k=r["top_k"])
            assert int(draw[0]) == tok, j
        # the penalty slot stopped at its first (wrong) draft; the vLLM slot took every row against counts that grew row by row
        assert len(out["history"][2]) == len(c.hist[2]) + 1 and len(out["history"][3]) == len(c.hist[3]) + K + 1
        assert out["history"][3][len(c.hist[3]):] == c.chain[3]


@pytest.mark.parametrize("K", [3, 15])
def test_eos_stop_stop_any_and_budget_inside_an_accepted_run(K):
    V = 1000
    probe = _Case(V, K, seed=99)
    hist = [5, 6, 7]
    probe.slot(dict(max_new_tokens=60, eos_token_id=-1), hist, K)
    chain = probe.build().chain[0]
    assert len(set(chain)) == K + 1 and not set(chain) & set(hist)
    j = 2                                                # the end falls on draft row 2
    for req, n_emit in ((dict(max_new_tokens=60, eos_token_id=chain[j]), j + 1),
                        (dict(max_new_tokens=60, eos_token_id=chain[j], min_new_tokens=len(hist) + j + 1), K + 1),       # held at its column
                        (dict(max_new_tokens=60, eos_token_id=-1, stop_ids=[chain[j - 1], chain[j]]), j + 1),
                        (dict(max_new_tokens=60, eos_token_id=-1, semantics="vllm", stop_any_ids=[999, chain[j]]), j + 1),
                        (dict(max_new_tokens=len(hist) + j + 1, eos_token_id=-1), j + 1)):
        c = _Case(V, K, seed=99)
        c.slot(req, hist, K)
        c.build()
        if req["max_new_tokens"] < 60:
            c.rows[0][j + 1:] = [c.rows[0][0]] * (K - j)          # a slot never drafts past its budget
            c.pos[0][j + 1:] = [c.pos[0][0]] * (K - j)
            c.nd[0] = j
        out = c.launch()
        c.check(out, c.restated())
        held = req.get("min_new_tokens", 0) > 0
        assert len(out["history"][0]) == len(hist) + n_emit and out["live"][0] == int(held) and out["finished"] == int(not held)
        if not held:
            assert out["history"][0][len(hist):] == chain[:n_emit] and out["n_draft"][0] == 0 and out["rows"][0] == [chain[j]] * (K + 1)


def test_a_row_of_nans_emits_id_0_and_raises_bad():
    V, K = 1000, 3
    c = _Case(V, K, seed=5)
    c.slot(dict(max_new_tokens=60, eos_token_id=-1), [4, 5], 0, lg=torch.full((K + 1, V), float("nan")))
    c.slot(dict(max_new_tokens=60, eos_token_id=-1), [4, 5], K)
    c.build()
    out = c.launch()
    c.check(out, c.restated())
    assert out["bad"] == 1 and out["history"][0] == [4, 5, 0] and out["live"] == [1, 1] and len(out["history"][1]) == 2 + K + 1


def test_forced_drafts_the_lookup_and_the_records():
    V, K = 1000, 3
    c = _Case(V, K, seed=11)
    hist = [3, 4, 3, 5, 6, 3, 4]
    c.slot(dict(max_new_tokens=60, eos_token_id=-1), hist, 0)
    c.slot(dict(max_new_tokens=len(hist) + 3, eos_token_id=-1), hist, 0)                       # budget: room for one draft only
    c.slot(dict(max_new_tokens=60, eos_token_id=-1, repetition_penalty=1.2), hist, K)
    c.build()
    forced = [[(7 * i + s) % V for i in range(20)] for s in range(2)]                            # slot 2 drafts by the lookup
    for mx, mn in ((0, 0), (1, 1), (8, 2)):
        out = c.launch(mx, mn, forced=forced)
        c.check(out, c.restated(mx or 3, mn or 1, forced=forced))
        L = len(out["history"][0])
        assert out["rows"][0][1:] == forced[0][L:L + K] and out["n_draft"][1] == 1
    # the records of the columns a slot emitted are the plain recording step's on the same rows and states
    lps = [dict(k=0, source="raw"), None, dict(k=0, source="processed")]
    out = c.launch(logprobs=lps)
    c.check(out, c.restated())
    for s in (0, 2):
        L0 = len(c.hist[s])
        emitted = out["history"][s][L0:]
        for j, tok in enumerate(emitted):
            t, lp, rk, _, _ = E.op_cb_logprobs(c.rows_lg[s][j:j + 1].to(dev()), [c.reqs[s]], [lps[s]], [c.hist[s] + emitted[:j]])
            assert int(t[0]) == tok
            assert torch.tensor([out["logprob"][s][j]]).view(torch.int32).item() == lp.view(torch.int32)[0].item() and out["rank"][s][j] == int(rk[0])
        assert all(v != v for v in out["logprob"][s][len(emitted):])
    assert all(v != v for v in out["logprob"][1])
