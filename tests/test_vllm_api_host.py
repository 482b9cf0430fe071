"""CPU: the vLLM-style offline API (star-vector_amd/vllm.py) -- SamplingParams' defaults and range checks (vLLM 0.5.5's
`_verify_args`), the mapping onto the continuous batch's request dicts, input parsing and output order over a scripted engine, the
ABI 9 request struct against the header, the device entry points' argument checks, and no CPU fallback."""
import ctypes as C
import os
import re
import threading

import pytest
import torch

from starvector_amd import vllm as V
from starvector_amd.engine import EngineConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- SamplingParams ------------------------------------------------------------------------------------------------------
def test_sampling_params_defaults_are_vllms():
    sp = V.SamplingParams()
    assert (sp.n, sp.best_of, sp.temperature, sp.top_p, sp.top_k, sp.min_p) == (1, 1, 1.0, 1.0, -1, 0.0)
    assert (sp.presence_penalty, sp.frequency_penalty, sp.repetition_penalty) == (0.0, 0.0, 1.0)
    assert (sp.seed, sp.max_tokens, sp.min_tokens, sp.stop_token_ids, sp.ignore_eos, sp.skip_special_tokens) == \
        (None, 16, 0, [], False, True)
    assert sp.logit_bias == {} and not sp.greedy


@pytest.mark.parametrize("kw", [
    dict(presence_penalty=2.5), dict(presence_penalty=-2.01), dict(frequency_penalty=2.01), dict(frequency_penalty=-3),
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1), dict(temperature=-0.1), dict(top_p=0.0), dict(top_p=1.01),
    dict(top_k=0), dict(top_k=-2), dict(min_p=-0.01), dict(min_p=1.5), dict(max_tokens=0), dict(min_tokens=-1),
    dict(max_tokens=4, min_tokens=5), dict(n=0), dict(temperature=0.0, n=2), dict(n=2, best_of=1),
    dict(stop_token_ids=list(range(9))), dict(logit_bias={i: 1.0 for i in range(129)}),
])
def test_sampling_params_range_checks(kw):
    with pytest.raises(ValueError):
        V.SamplingParams(**kw)


@pytest.mark.parametrize("kw", [dict(n=1, best_of=2), dict(logprobs=1), dict(prompt_logprobs=0), dict(stop="</svg>"),
                                dict(stop=["a"]), dict(use_beam_search=True)])
def test_sampling_params_unbuilt_fields_raise(kw):
    with pytest.raises(NotImplementedError):
        V.SamplingParams(**kw)


def test_sampling_params_edges_accepted():
    for kw in (dict(presence_penalty=2.0, frequency_penalty=-2.0), dict(top_p=1.0, top_k=1), dict(min_p=1.0),
               dict(max_tokens=3, min_tokens=3), dict(temperature=0.0), dict(max_tokens=None), dict(n=4, temperature=0.7)):
        V.SamplingParams(**kw)


# ---- mapping onto the request dicts --------------------------------------------------------------------------------------
def _req(sp, seed=7, max_new=10, prompt=(5, 6), eos=0, pad=3, vocab=100):
    return V.request_params(sp, seed, max_new, list(prompt), eos, pad, vocab)


def test_greedy_neutralises_the_warpers():
    sp = V.SamplingParams(temperature=0.0, top_p=0.5, top_k=7, min_p=0.3, presence_penalty=0.5)
    assert (sp.top_p, sp.top_k, sp.min_p) == (1.0, -1, 0.0)
    r = _req(sp)
    assert r["do_sample"] is False and r["top_k"] == 0 and r["top_p"] == 1.0 and r["min_p"] == 0.0 and r["temperature"] == 1.0
    assert r["presence_penalty"] == 0.5 and r["semantics"] == "vllm"
    assert _req(V.SamplingParams(temperature=0.9e-5))["do_sample"] is False


def test_sampling_fields_map_through():
    sp = V.SamplingParams(temperature=0.8, top_p=0.95, top_k=-1, min_p=0.05, frequency_penalty=0.3, presence_penalty=-0.2,
                          repetition_penalty=1.1, min_tokens=4, stop_token_ids=[9, 11])
    r = _req(sp, seed=123, max_new=50, prompt=(1, 2, 2))
    assert r["do_sample"] is True and r["temperature"] == 0.8 and r["top_p"] == 0.95 and r["top_k"] == 0
    assert abs(r["min_p"] - 0.05) < 1e-12 and r["frequency_penalty"] == 0.3 and r["presence_penalty"] == -0.2
    assert r["repetition_penalty"] == 1.1 and r["min_new_tokens"] == 4 and r["stop_any_ids"] == [9, 11]
    assert r["prompt_ids"] == [1, 2, 2] and r["max_new_tokens"] == 50 and r["seed"] == 123 and r["eos_token_id"] == 0
    assert _req(V.SamplingParams(top_k=40))["top_k"] == 40
    assert _req(V.SamplingParams(ignore_eos=True))["eos_token_id"] == -1


def test_logit_bias_is_clamped_and_checked():
    r = _req(V.SamplingParams(logit_bias={5: 250.0, 6: -1e9, 7: 1.5}))
    assert r["logit_bias"] == {5: 100.0, 6: -100.0, 7: 1.5}
    with pytest.raises(ValueError):
        _req(V.SamplingParams(logit_bias={100: 1.0}), vocab=100)
    with pytest.raises(ValueError):
        _req(V.SamplingParams(logit_bias={-1: 1.0}))
    with pytest.raises(ValueError):
        _req(V.SamplingParams(stop_token_ids=[100]), vocab=100)


def test_seeds_distinct_and_reproducible():
    sp = V.SamplingParams(n=4, seed=42, temperature=0.7)
    a, b = V.sample_seeds(sp), V.sample_seeds(V.SamplingParams(n=4, seed=42, temperature=0.7))
    assert a == b and len(set(a)) == 4 and all(0 <= s < 2 ** 63 for s in a)
    assert V.sample_seeds(V.SamplingParams(n=4, seed=43, temperature=0.7)) != a
    un = V.SamplingParams(n=3, temperature=0.7)
    torch.manual_seed(5)
    x = V.sample_seeds(un)
    torch.manual_seed(5)
    assert V.sample_seeds(un) == x and len(set(x)) == 3
    assert V.sample_seeds(un) != x


def test_finish_reasons():
    sp = V.SamplingParams(stop_token_ids=[7])
    assert V.finish_of([4, 5, 0], sp, 0) == ("stop", None, 2)
    assert V.finish_of([4, 7], sp, 0) == ("stop", 7, 1)
    assert V.finish_of([4, 5], sp, 0) == ("length", None, 2)
    assert V.finish_of([4, 0], V.SamplingParams(ignore_eos=True), 0) == ("length", None, 2)


# ---- inputs and outputs --------------------------------------------------------------------------------------------------
def test_parse_inputs_forms():
    sp1, sp2 = V.SamplingParams(seed=1), V.SamplingParams(seed=2)
    img = object()
    assert V.parse_inputs("abc", None)[0][:2] == ("abc", None)
    got = V.parse_inputs([{"prompt": "<image-start>", "multi_modal_data": {"image": img}}, "x"], [sp1, sp2])
    assert [(p, i is img, s) for p, i, s in got] == [("<image-start>", True, sp1), ("x", False, sp2)]
    assert [s for _, _, s in V.parse_inputs(["a", "b", "c"], sp1)] == [sp1] * 3
    assert V.parse_inputs({"prompt": "q"}, sp1) == [("q", None, sp1)]
    with pytest.raises(ValueError):
        V.parse_inputs(["a", "b"], [sp1])
    with pytest.raises(ValueError):
        V.parse_inputs([{"multi_modal_data": {}}], sp1)
    with pytest.raises(NotImplementedError):
        V.parse_inputs([{"prompt": "a", "multi_modal_data": {"audio": 1}}], sp1)
    with pytest.raises(TypeError):
        V.parse_inputs([3], sp1)


class _Tok:
    eos_token_id, pad_token_id = 0, 99

    def decode(self, ids, skip_special_tokens=True):
        return ",".join(str(t) for t in ids)


class _ScriptedEngine:
    """sv_cb_* surface on the host: a request whose prompt embedding holds m emits m, m+1, ... for max_new_tokens tokens
    (or until its eos / a stop id); slots are few, so the batcher queues."""
    device = 0

    def __init__(self, max_batch=2):
        self.cfg = EngineConfig(image_size=28, patch_size=14, vit_width=4, hidden=8, vocab=1000, max_batch=max_batch, max_seq_len=64)
        self.slots, self.lock, self.seen = {}, threading.Lock(), []

    def cb_admit(self, emb, reqs):
        from starvector_amd._lib import StarVectorBusy
        with self.lock:
            free = [s for s in range(self.cfg.max_batch) if s not in self.slots]
            if len(free) < len(reqs):
                raise StarVectorBusy("busy")
            out = []
            for i, r in enumerate(reqs):
                self.seen.append(r)
                m = int(emb[i, 0, 0])
                v = dict(toks=[m], r=r)
                v["live"] = not self._done(v)
                self.slots[free[i]] = v
                out.append(free[i])
            return out

    @staticmethod
    def _done(v):
        t, r = v["toks"][-1], v["r"]
        return len(v["toks"]) >= r["max_new_tokens"] or t == r["eos_token_id"] or t in r["stop_any_ids"]

    def cb_step(self, n):
        with self.lock:
            for _ in range(n):
                for v in self.slots.values():
                    if v["live"]:
                        v["toks"].append(v["toks"][-1] + 1)
                        v["live"] = not self._done(v)
            return sum(v["live"] for v in self.slots.values())

    def cb_poll(self):
        with self.lock:
            n = self.cfg.max_batch
            return ([int(self.slots[s]["live"]) if s in self.slots else 0 for s in range(n)],
                    [len(self.slots[s]["toks"]) if s in self.slots else 0 for s in range(n)])

    def cb_read(self, slot, first, count):
        with self.lock:
            return torch.tensor(self.slots[slot]["toks"][first:first + count], dtype=torch.int64)

    def cb_release(self, slot):
        with self.lock:
            del self.slots[slot]

    def cb_reset(self):
        with self.lock:
            self.slots.clear()


def _scripted_llm(max_batch=2):
    llm = V.LLM.__new__(V.LLM)
    llm.engine, llm.tokenizer, llm.max_model_len = _ScriptedEngine(max_batch), _Tok(), 64
    llm._ids = iter(range(10 ** 6))

    def embed(prompt, image):                         # the prompt text's first character's code starts the stream
        m = int(prompt)
        return [m, m], torch.full((1, 2, 8), float(m))
    llm._embed = embed
    return llm


def test_generate_returns_input_order_with_n_samples():
    llm = _scripted_llm(max_batch=2)
    sps = [V.SamplingParams(n=2, seed=1, max_tokens=3), V.SamplingParams(max_tokens=5, stop_token_ids=[13]),
           V.SamplingParams(n=2, seed=3, max_tokens=4, temperature=0.5), V.SamplingParams(max_tokens=2, ignore_eos=True)]
    outs = llm.generate(["50", "10", "30", "70"], sps)
    assert [o.prompt for o in outs] == ["50", "10", "30", "70"] and all(o.finished for o in outs)
    assert [o.prompt_token_ids for o in outs] == [[50, 50], [10, 10], [30, 30], [70, 70]]
    assert [[c.index for c in o.outputs] for o in outs] == [[0, 1], [0], [0, 1], [0]]
    assert outs[0].outputs[1].token_ids == [50, 51, 52] and outs[0].outputs[1].finish_reason == "length"
    assert outs[1].outputs[0].token_ids == [10, 11, 12, 13]
    assert (outs[1].outputs[0].finish_reason, outs[1].outputs[0].stop_reason, outs[1].outputs[0].text) == ("stop", 13, "10,11,12")
    assert outs[3].outputs[0].text == "70,71" and outs[3].outputs[0].stop_reason is None
    assert len(set(o.request_id for o in outs)) == 4
    seeds = [r["seed"] for r in llm.engine.seen if r["prompt_ids"] == [50, 50]]
    assert seeds == V.sample_seeds(sps[0])
    assert all(r["semantics"] == "vllm" for r in llm.engine.seen) and len(llm.engine.seen) == 6


def test_generate_clamps_max_tokens_to_the_model_length():
    llm = _scripted_llm()
    llm.max_model_len = 6                              # prompt 2 -> at most 4 new tokens
    out = llm.generate("100", V.SamplingParams(max_tokens=50))
    assert out[0].outputs[0].token_ids == [100, 101, 102, 103]
    llm.max_model_len = 2
    with pytest.raises(ValueError):
        llm.generate("100", V.SamplingParams())


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def _header_fields(struct):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "starvector_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            parts = decl.split(",")
            out.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", parts[0])[-1])
            out += [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", x)[-1] for x in parts[1:]]
    return out


def test_cb_request_struct_matches_header():
    from starvector_amd import _lib
    names = [f[0] for f in _lib.SvCbRequest._fields_]
    assert _header_fields("sv_cb_request") == names
    assert names[:12] == ["do_sample", "temperature", "top_p", "top_k", "seed", "max_new_tokens", "eos_token_id", "pad_token_id",
                          "min_new_tokens", "repetition_penalty", "n_stop", "stop_ids"]          # ABI 8's prefix, unchanged
    assert names[12:] == ["semantics", "presence_penalty", "frequency_penalty", "min_p", "n_prompt_ids", "prompt_ids",
                          "n_logit_bias", "logit_bias_ids", "logit_bias_values", "n_stop_any", "stop_any_ids"]
    assert _lib.SvCbRequest.stop_ids.offset == 48 and _lib.SvCbRequest.semantics.offset == 112
    assert _lib.ABI_VERSION == 9
    assert "#define SV_ABI_VERSION 9" in open(os.path.join(ROOT, "include", "starvector_hip.h")).read()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from starvector_amd import _lib
    return _lib.load()


def test_cb_request_validation_precedes_device_work(lib):
    """sv_op_cb_select runs sv_cb_admit's request checks before it touches the GPU: a vLLM field under HF semantics, ids
    outside the vocabulary, caps exceeded and duplicate bias ids are SV_EINVAL with a message."""
    from starvector_amd import engine as E

    def call(**r):
        arr, keep = E.cb_requests([dict(dict(max_new_tokens=4), **r)])
        hl = (C.c_int32 * 1)(0)
        out = (C.c_int32 * 1)()
        rc = lib.sv_op_cb_select(C.c_void_p(16), 1, 100, 100, arr, None, 0, hl, out, None)
        return rc, lib.sv_last_error().decode()

    for field, val in [("min_p", 0.1), ("presence_penalty", 0.5), ("frequency_penalty", -0.5), ("prompt_ids", [1]),
                       ("logit_bias", {3: 1.0}), ("stop_any_ids", [4])]:
        rc, msg = call(**{field: val})
        assert rc == -22 and field.split("_ids")[0] in msg and "semantics" in msg, (field, msg)
    for r, what in [(dict(prompt_ids=[100]), "prompt id"), (dict(logit_bias={100: 1.0}), "logit_bias id"),
                    (dict(stop_any_ids=[-1]), "stop id"), (dict(min_p=1.5), "min_p"), (dict(max_new_tokens=70000), "16 bits"),
                    (dict(frequency_penalty=float("inf")), "finite"), (dict(eos_token_id=100), "eos_token_id")]:
        rc, msg = call(semantics="vllm", **r)
        assert rc == -22 and what in msg, (r, msg)
    arr, keep = E.cb_requests([dict(max_new_tokens=4, semantics="vllm")])
    arr[0].semantics = 2
    rc = lib.sv_op_cb_select(C.c_void_p(16), 1, 100, 100, arr, None, 0, (C.c_int32 * 1)(0), (C.c_int32 * 1)(), None)
    assert rc == -22 and "semantics" in lib.sv_last_error().decode()
    ids, vals = (C.c_int32 * 2)(5, 5), (C.c_float * 2)(1.0, 2.0)
    arr[0].semantics, arr[0].n_logit_bias = 1, 2
    arr[0].logit_bias_ids, arr[0].logit_bias_values = C.cast(ids, C.POINTER(C.c_int32)), C.cast(vals, C.POINTER(C.c_float))
    rc = lib.sv_op_cb_select(C.c_void_p(16), 1, 100, 100, arr, None, 0, (C.c_int32 * 1)(0), (C.c_int32 * 1)(), None)
    assert rc == -22 and "twice" in lib.sv_last_error().decode()
    with pytest.raises(ValueError):
        E.cb_requests([dict(max_new_tokens=4, semantics="vllm", logit_bias={i: 1.0 for i in range(129)})])
    with pytest.raises(ValueError):
        E.cb_requests([dict(max_new_tokens=4, semantics="openai")])


def test_llm_has_no_cpu_fallback(tmp_path):
    import starvector_amd as sva
    from oracle import starvector_oracle as O
    from tests.ckpt_util import write_reference_checkpoint
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    cfg = O.OracleConfig.tiny()
    write_reference_checkpoint(str(tmp_path / "ckpt"), cfg, O.make_weights(cfg, seed=0))
    with pytest.raises(sva.StarVectorHipError):
        V.LLM(model=str(tmp_path / "ckpt"), max_num_seqs=2, byte_tokenizer_fallback=True)
    with pytest.raises(FileNotFoundError):
        V.LLM(model="starvector/starvector-1b-im2svg")
