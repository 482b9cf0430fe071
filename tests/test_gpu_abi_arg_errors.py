"""GPU: the refusals of the generate, scoring and continuous-batch admit entry points that lie BEHIND the engine check -- they need an
engine's max_batch, max_seq_len and vocabulary, or its state -- through the C ABI, code and full message text.  The companion of
tests/test_abi_arg_errors_host.py, which pins what comes in front of the engine check.  Nothing here is meant to reach a kernel that can
fail: the only launches are those of the two scoring calls (whose kernels find the bad target) and of one successful admit."""
import ctypes as C

import pytest
import torch

from starvector_amd import _lib
from starvector_amd import engine as E
from tests.gpu_util import dev
from tests.test_gpu_ragged_prefill import _tiny_engine

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EBUSY = -22, -1, -16
BUSY = " a continuous batch holds the KV cache of this engine (sv_cb_reset first)"


def test_refusals_behind_the_engine_check_keep_code_and_text():
    cfg, eng = _tiny_engine("v1", max_batch=4, max_seq_len=128)
    lib, h, V, D = eng.lib, eng._h, cfg.vocab, cfg.hidden
    assert (V, eng.cfg.max_batch, eng.cfg.max_seq_len) == (516, 4, 128)
    x = (torch.randn(5 * 129, D, generator=torch.Generator().manual_seed(5)) * 0.5).to(torch.bfloat16).to(dev())      # embeddings for every call below
    buf = torch.zeros(1 << 16, dtype=torch.float32, device=dev())                                                     # any output
    X, O, n_gen = C.c_void_p(x.data_ptr()), C.c_void_p(buf.data_ptr()), C.c_int32(0)
    ints = lambda *v: (C.c_int32 * len(v))(*v)

    def sampling(max_length=14, **kw):
        return _lib.SvSampling(**dict(dict(max_length=max_length, num_beams=1, temperature=1.0, top_p=1.0, eos_token_id=-1), **kw))

    def expect(rc, code, text):
        assert (rc, lib.sv_last_error().decode()) == (code, text)

    def generate(B=2, S0=4, sp=None):
        return lib.sv_generate(h, X, B, S0, C.byref(sp or sampling()), O, C.byref(n_gen), None)

    def shared(B, lens, S0, G):
        return lib.sv_generate_shared(h, X, B, lens, S0, G, C.byref(sampling(140 if lens else 14)), None, O, C.byref(n_gen), None)

    def score(entry, B=2, S=5, n_keep=3, lens=(3, 5), keep=(2, 3), targets=O, k=0):
        lists = (k, O, O, O) if entry != "sv_forward_logprobs" else ()
        shape = (ints(*lens), ints(*keep)) if entry == "sv_forward_logprobs_ragged" else (S, n_keep)
        return getattr(lib, entry)(h, X, B, *shape, targets, 1.0, O, O, None, None, *lists, None)

    def admit(entry, n=2, S0=4, lens=(4, 4), group=(0, 1), budget=4):
        reqs, _keep = E.cb_requests([dict(max_new_tokens=budget, eos_token_id=-1)] * n)
        slots = (C.c_int32 * n)()
        if entry == "sv_cb_admit":
            return lib.sv_cb_admit(h, X, n, S0, reqs, slots, None), list(slots)
        if entry == "sv_cb_admit_ragged":
            return lib.sv_cb_admit_ragged(h, X, n, ints(*lens), reqs, slots, None), list(slots)
        lps = (None,) if entry == "sv_cb_admit_logprobs" else ()
        return getattr(lib, entry)(h, X, len(lens), ints(*lens), n, ints(*group), reqs, *lps, slots, None), list(slots)

    ADMITS = ("sv_cb_admit", "sv_cb_admit_ragged", "sv_cb_admit_shared", "sv_cb_admit_logprobs")
    SCORES = ("sv_forward_logprobs", "sv_forward_topk", "sv_forward_logprobs_ragged")
    try:
        # ---- B above max_batch, every family; B x n_samples
        expect(generate(B=5), EINVAL, "prefill: bad B=5 (max_batch 4)")
        expect(lib.sv_generate_ragged(h, X, 5, ints(3, 3, 3, 3, 3), C.byref(sampling()), None, O, C.byref(n_gen), None), EINVAL,
               "sv_generate_ragged: bad B=5 (max_batch 4)")
        expect(shared(2, None, 4, 3), EINVAL, "sv_generate_shared: B 2 x n_samples 3 exceeds engine max_batch 4")
        expect(shared(5, None, 4, 1), EINVAL, "prefill: bad B=5 (max_batch 4)")
        expect(lib.sv_forward_logits(h, X, 5, 5, 3, O, None), EINVAL, "sv_forward_logits: bad B=5 (max_batch 4)")
        for entry in SCORES:
            expect(score(entry, B=5, lens=(3,) * 5, keep=(2,) * 5, k=4 if entry == "sv_forward_topk" else 0), EINVAL,
                   f"{entry}: bad B=5 (max_batch 4)")
        for entry in ADMITS:
            expect(admit(entry, n=5, lens=(4,) * 5, group=(0, 1, 2, 3, 4))[0], EINVAL, f"{entry}: 5 requests exceed max_batch 4")
        # ---- a length above max_seq_len
        expect(lib.sv_generate_ragged(h, X, 2, ints(3, 129), C.byref(sampling(140)), None, O, C.byref(n_gen), None), EINVAL,
               "sv_generate_ragged: length 129 of sequence 1 out of range (1..max_seq_len 128)")
        expect(shared(2, ints(3, 129), 0, 2), EINVAL, "sv_generate_shared: length 129 of sequence 1 out of range (1..max_seq_len 128)")
        expect(lib.sv_forward_logits(h, X, 2, 129, 3, O, None), EINVAL, "sv_forward_logits: S=129 out of range (max_seq_len 128)")
        expect(score("sv_forward_logprobs", S=129), EINVAL, "sv_forward_logprobs: S=129 out of range (max_seq_len 128)")
        expect(score("sv_forward_topk", S=129, k=4), EINVAL, "sv_forward_topk: S=129 out of range (max_seq_len 128)")
        expect(score("sv_forward_logprobs_ragged", lens=(3, 129)), EINVAL,
               "sv_forward_logprobs_ragged: length 129 of sequence 1 out of range (1..max_seq_len 128)")
        expect(admit("sv_cb_admit", S0=125)[0], EINVAL, "sv_cb_admit: request 0: prompt 125 + max_new_tokens 4 out of range (max_seq_len 128)")
        expect(admit("sv_cb_admit_ragged", lens=(4, 129))[0], EINVAL,
               "sv_cb_admit_ragged: request 1: prompt 129 + max_new_tokens 4 out of range (max_seq_len 128)")
        for entry in ADMITS[2:]:
            expect(admit(entry, lens=(4, 126))[0], EINVAL, f"{entry}: request 1: prompt 126 + max_new_tokens 4 out of range (max_seq_len 128)")
            expect(admit(entry, budget=0)[0], EINVAL, f"{entry}: request 0: prompt 4 + max_new_tokens 0 out of range (max_seq_len 128)")
        # ---- the budget, the stop sequence, the outputs' row length
        expect(generate(sp=sampling(4)), EINVAL, "max_length (4) must exceed the prompt length (4)")
        expect(generate(sp=sampling(129)), EINVAL, "max_length 129 exceeds engine max_seq_len 128")
        expect(generate(sp=sampling(n_stop=17)), EINVAL, "stop sequence length 17 unsupported (0..16)")
        outs = _lib.SvGenerateOutputs(dev_scores=O, ld=V - 1)
        expect(lib.sv_generate_ex(h, X, 2, 4, C.byref(sampling()), C.byref(outs), O, C.byref(n_gen), None), EINVAL,
               "sv_generate_ex: ld 515 must be >= vocab 516")
        # ---- a target id outside the vocabulary, found by the scoring kernels: packed kept row 4 in both forms.  B = 2, S = 5, n_keep = 3: row 4 is
        # sequence 1, kept position 1; lengths (3, 5), keep (2, 3): sequence 1 begins at row 2, so row 4 is its kept position 2
        tg = torch.tensor([1, 2, 3, 4, V, 5], dtype=torch.int32, device=dev())
        T = C.c_void_p(tg.data_ptr())
        expect(score("sv_forward_topk", targets=T, k=3), EINVAL,
               "sv_forward_topk: a target id outside [0, 516) that is not -100; first at row 4 (sequence 1, kept position 1)")
        expect(score("sv_forward_logprobs_ragged", targets=T), EINVAL,
               "sv_forward_logprobs_ragged: a target id outside [0, 516) that is not -100; first at row 4 (sequence 1, kept position 2)")
        # ---- 2 requests in, 3 more do not fit into the 4 slots: SV_EBUSY, nothing taken
        rc, slots = admit("sv_cb_admit")
        assert rc == 0 and slots == [0, 1], lib.sv_last_error()
        free, total = eng.free_pages()
        assert free == total - 2
        rc, slots = admit("sv_cb_admit", n=3)
        expect(rc, EBUSY, f"sv_cb_admit: 3 requests need 3 slots / 3 KV pages, 2 / {free} are free (release finished slots first)")
        assert eng.free_pages() == (free, total)
        rc, slots = admit("sv_cb_admit_shared", n=3, lens=(4,), group=(0, 0, 0))
        expect(rc, EBUSY, f"sv_cb_admit_shared: 3 requests over 1 prompts need 3 slots / 3 KV pages, 2 / {free} are free (release finished slots first)")
        assert eng.free_pages() == (free, total)
        # ---- a continuous batch holds the cache: every generate and scoring call is refused
        expect(generate(), ESTATE, "sv_generate:" + BUSY)
        expect(lib.sv_generate_ragged(h, X, 2, ints(3, 5), C.byref(sampling()), None, O, C.byref(n_gen), None), ESTATE, "sv_generate:" + BUSY)
        expect(shared(2, None, 4, 2), ESTATE, "sv_generate:" + BUSY)
        expect(lib.sv_forward_logits(h, X, 2, 5, 3, O, None), ESTATE, "sv_forward_logits:" + BUSY)
        for entry in SCORES:
            expect(score(entry, k=4 if entry == "sv_forward_topk" else 0), ESTATE, f"{entry}:" + BUSY)
    finally:
        eng.cb_reset()
        eng.close()
