"""Continuous batching on the host side.

The reference's worker lets 5 requests in at a time (serve/model_worker.py:161-172,216-229: an asyncio semaphore around
`generate_stream`) and runs each as its own HF `generate` call on its own thread; on one GPU those calls simply take turns.
Here concurrent requests share ONE decode loop: `ContinuousBatcher` owns a scheduler thread that

  * admits waiting requests into free rows ("slots") of the engine's batch -- a prompt pass for the newcomers only, while the
    running requests keep their KV pages (`sv_cb_admit`),
  * advances every live slot by a few decode steps per iteration (`sv_cb_step`: one captured hipGraph per row bucket),
  * hands each request the tokens that became final since the last look (streaming) and frees the slots of finished requests.

A request whose params carry ``logprobs`` (k, 0..32) records on device, per emitted token, the token's log-prob and rank and the k most
likely ids (`sv_cb_admit_logprobs`; ``logprob_source`` "raw" | "processed", default: processed under vLLM semantics, raw otherwise); the
record arrives with the tokens and `_Request.logprobs` holds it.  Requests without the key are queued and admitted as before.

Every slot has its own sampling parameters, budget, EOS, stop sequence and random stream, so a request's tokens are exactly
what a solo `HipEngine.generate` call would return for it (tests/test_gpu_serving.py).  No kernels here: host logic only.

``prompt_lookup_num_tokens=K`` switches on prompt-lookup drafting for the whole batch (`HipEngine.cb_set_lookup`): a step verifies up to K
drafted tokens per request and emits 1 .. K + 1 of them, the tokens of every request stay what they are without it, and the batch holds
max_batch // (K + 1) requests -- at the reference worker's 5 concurrent requests the other rows of a 32- or 64-row engine are idle anyway.

``prefix_cache=True`` switches on the engine's prefix cache for the batch (`HipEngine.cb_set_prefix_cache`): the full KV pages of a prompt stay
findable -- by digests of its embedding rows -- after its request has left, and a later request with the same leading rows (the same image
again, the next part of a group that did not fit at once, the next temperature of a sweep) computes only what lies behind them.  Same tokens.
"""
from __future__ import annotations

import threading
from collections import deque
from typing import Callable, Deque, Dict, List, NamedTuple, Optional

import torch

from ._lib import StarVectorBusy


class TokenLogprobs(NamedTuple):
    """The record of a request that asked for ``logprobs``, N = tokens emitted: log-prob and rank of each, the k best ids and their log-probs."""
    logprobs: torch.Tensor           # fp32 [N]
    ranks: torch.Tensor              # int32 [N]
    top_ids: torch.Tensor            # int32 [N, k], -1 past the ids that enter
    top_logprobs: torch.Tensor       # fp32 [N, k], -inf there


def _logprobs_of(params: dict) -> Optional[dict]:
    """What a request's params ask the engine to record: None, or the `HipEngine.cb_admit` logprobs entry."""
    k = params.get("logprobs")
    if k is None or k is False:
        return None
    return dict(k=int(k), source=params.get("logprob_source"))


class _Request:
    def __init__(self, emb: Optional[torch.Tensor], params: dict, on_tokens: Optional[Callable], exclusive: Optional[Callable] = None):
        self.emb, self.params, self.on_tokens = emb, params, on_tokens
        self.exclusive = exclusive         # a callable that needs the engine to itself (beam search, scoring forward)
        self.group = None                  # submit_group: the requests that sample the same prompt carry the same token
        self.value = None
        self.slot: Optional[int] = None
        self.sent = 0                      # tokens already handed over
        self.chunks: List[torch.Tensor] = []
        self.lp = _logprobs_of(params)     # None: the request records no log-probs
        self.lp_chunks: List[tuple] = []
        self.done = threading.Event()
        self.error: Optional[BaseException] = None

    def result(self, timeout: Optional[float] = None) -> torch.Tensor:
        """Blocks until the request has finished; int64 [1, N] new tokens (HF `generate` shape for one sequence)."""
        if not self.done.wait(timeout):
            raise TimeoutError("generation did not finish in time")
        if self.error is not None:
            raise self.error
        if self.exclusive is not None:
            return self.value
        toks = torch.cat(self.chunks) if self.chunks else torch.empty(0, dtype=torch.int64)
        return toks.view(1, -1)

    @property
    def logprobs(self) -> Optional[TokenLogprobs]:
        """The record delivered so far (complete once `result` returns); None for a request that did not ask."""
        if self.lp is None:
            return None
        if not self.lp_chunks:
            k = self.lp["k"]
            return TokenLogprobs(torch.empty(0), torch.empty(0, dtype=torch.int32), torch.empty(0, k, dtype=torch.int32), torch.empty(0, k))
        return TokenLogprobs(*[torch.cat(c) for c in zip(*self.lp_chunks)])


class ContinuousBatcher:
    """engine: a `HipEngine` (or anything with cb_admit / cb_step / cb_poll / cb_read / cb_release / cb_reset and `.cfg`)."""

    def __init__(self, engine, steps_per_poll: int = 8, device: Optional[int] = None, prompt_lookup_num_tokens: int = 0,
                 max_matching_ngram_size: int = 0, min_matching_ngram_size: int = 0, prefix_cache: bool = False):
        self.engine = engine
        self.steps_per_poll = int(steps_per_poll)
        self.device = getattr(engine, "device", 0) if device is None else device
        # prompt-lookup drafting (sv_cb_set_lookup): K > 0 -- set before the first admit -- makes every step verify up to K drafted tokens per
        # request; a slot then owns K + 1 decode rows, so the batch holds max_batch // (K + 1) requests and the rest waits in the queue
        self.lookup_k = int(prompt_lookup_num_tokens or 0)
        if self.lookup_k < 0:
            raise ValueError("prompt_lookup_num_tokens must be >= 0")
        self.slots = int(engine.cfg.max_batch) // (self.lookup_k + 1)
        if self.lookup_k:
            if self.slots < 1:
                raise NotImplementedError(f"prompt_lookup_num_tokens {self.lookup_k} + 1 rows per request exceed max_batch {engine.cfg.max_batch}")
            engine.cb_reset()
            engine.cb_set_lookup(self.lookup_k, int(max_matching_ngram_size or 0), int(min_matching_ngram_size or 0))
        # the prefix cache (sv_cb_set_prefix_cache), set before the first admit like the drafting: a prompt whose leading rows an earlier
        # request of the batch brought reuses that request's full KV pages and computes only the rows behind them -- the same tokens
        self.prefix_cache = bool(prefix_cache)
        if self.prefix_cache:
            engine.cb_reset()
            engine.cb_set_prefix_cache(True)
        self._lock = threading.Condition()
        self._pending: Deque[_Request] = deque()
        self._active: Dict[int, _Request] = {}
        self._closing = False
        self.max_concurrent = 0            # high-water mark of requests sharing the decode loop (tests, status)
        self.steps_run = 0
        self._thread = threading.Thread(target=self._loop, name="sv-continuous-batcher", daemon=True)
        self._thread.start()

    # ---- producer side -------------------------------------------------------------------------------------------------
    def submit(self, inputs_embeds: torch.Tensor, params: dict, on_tokens: Optional[Callable] = None) -> _Request:
        """inputs_embeds [1, S0, D]; params: the keys of `HipEngine.cb_admit` (max_new_tokens required);
        on_tokens(tokens int64 [k], first_index) is called from the scheduler thread as tokens become final."""
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[0] != 1:
            raise ValueError("one sequence per request: inputs_embeds must be [1, S0, D]")
        if int(params.get("max_new_tokens", 0)) < 1:
            raise ValueError("max_new_tokens must be >= 1")
        req = _Request(inputs_embeds, dict(params), on_tokens)
        with self._lock:
            if self._closing:
                raise RuntimeError("the batcher is closed")
            self._pending.append(req)
            self._lock.notify_all()
        return req

    def submit_group(self, inputs_embeds: torch.Tensor, params_list, on_tokens: Optional[Callable] = None) -> List[_Request]:
        """Several samples of ONE prompt: inputs_embeds [1, S0, D], one params dict per sample (own seed, budget, sampler).  Returns one
        handle per sample, each what `submit` returns.  Where the engine offers `cb_admit_shared` the samples that are admitted together
        share one prompt pass and the prompt's full KV pages; a group larger than the free slots (or than max_batch) is admitted in parts
        as slots and pages come free -- each part shares among itself -- so it never waits for all its slots at once."""
        if inputs_embeds.dim() != 3 or inputs_embeds.shape[0] != 1:
            raise ValueError("one prompt per group: inputs_embeds must be [1, S0, D]")
        params_list = [dict(p) for p in params_list]
        if not params_list or any(int(p.get("max_new_tokens", 0)) < 1 for p in params_list):
            raise ValueError("a group needs at least one sample, each with max_new_tokens >= 1")
        token = object()
        reqs = [_Request(inputs_embeds, p, on_tokens) for p in params_list]
        for r in reqs:
            r.group = token
        with self._lock:
            if self._closing:
                raise RuntimeError("the batcher is closed")
            self._pending.extend(reqs)
            self._lock.notify_all()
        return reqs

    def generate(self, inputs_embeds: torch.Tensor, params: dict, on_tokens: Optional[Callable] = None,
                 timeout: Optional[float] = None) -> torch.Tensor:
        return self.submit(inputs_embeds, params, on_tokens).result(timeout)

    def run_exclusive(self, fn: Callable, timeout: Optional[float] = None):
        """Run `fn()` with the engine to itself: what the slots cannot express (beam search keeps its own search state in
        the batch rows, the scoring forward wants the whole KV pool).  FIFO with the generation requests: the ones admitted
        before it finish first, the ones behind it wait; the continuous batch is reset around the call."""
        req = _Request(None, {}, None, exclusive=fn)
        with self._lock:
            if self._closing:
                raise RuntimeError("the batcher is closed")
            self._pending.append(req)
            self._lock.notify_all()
        return req.result(timeout)

    def lookup_counts(self) -> dict:
        """{steps, drafted, accepted} of the running batch since it began (sv_cb_lookup_counts, slot -1; steps: one per live request and
        step); zeros while drafting is off.  The engine starts a new batch -- and the totals from zero -- whenever it has run empty and was reset."""
        if not self.lookup_k:
            return {"steps": 0, "drafted": 0, "accepted": 0}
        return self.engine.cb_lookup_counts(-1)

    def prefix_cache_info(self) -> dict:
        """`HipEngine.cb_prefix_cache_info` of the running batch; zeros while the cache is off."""
        if not self.prefix_cache:
            return {"lookups": 0, "reused": 0, "resident": 0, "unheld": 0, "evictions": 0}
        return self.engine.cb_prefix_cache_info()

    def queue_length(self) -> int:
        with self._lock:
            return len(self._pending) + len(self._active)

    def close(self):
        with self._lock:
            self._closing = True
            self._lock.notify_all()
        self._thread.join(timeout=30)

    # ---- scheduler thread ----------------------------------------------------------------------------------------------
    def _admit(self) -> int:
        """Move waiting requests into free slots: ONE `cb_admit` -- one ragged prompt pass -- for all of them whatever their prompt
        lengths where the engine offers it (`prefill_ragged`), else one `cb_admit` per prompt length (the rectangular prompt pass).
        Returns how many requests left the queue (admitted, or failed alone)."""
        moved = 0
        with self._lock:
            waiting = []
            for r in self._pending:                 # FIFO up to the first exclusive job: nothing overtakes it
                if r.exclusive is not None:
                    break
                waiting.append(r)
        ragged = hasattr(self.engine, "prefill_ragged")
        by_len: Dict[int, List[_Request]] = {}
        for r in waiting:
            by_len.setdefault(0 if ragged else int(r.emb.shape[1]), []).append(r)
        for S0, group in by_len.items():
            room = self.slots - len(self._active)
            group = group[:room]
            while group:
                try:
                    # the requests that record log-probs ride in a keyword the engine sees only when one of them asks
                    kw = dict(logprobs=[r.lp for r in group]) if any(r.lp is not None for r in group) else {}
                    keys = [id(r) if r.group is None else id(r.group) for r in group]
                    prompts = list(dict.fromkeys(keys))         # in the order of their first request
                    if ragged and len(prompts) < len(group) and hasattr(self.engine, "cb_admit_shared"):
                        # samples of one prompt among them: one prompt pass per PROMPT, its full KV pages shared (sv_cb_admit_shared)
                        first = {k: r for r, k in reversed(list(zip(group, keys)))}
                        slots = self.engine.cb_admit_shared([first[k].emb[0] for k in prompts], None, [prompts.index(k) for k in keys],
                                                            [r.params for r in group], **kw)
                    elif ragged:
                        slots = self.engine.cb_admit([r.emb[0] for r in group], [r.params for r in group], **kw)
                    else:
                        slots = self.engine.cb_admit(torch.cat([r.emb for r in group], 0), [r.params for r in group], **kw)
                except StarVectorBusy:
                    group = group[:-1]              # KV pages are short: try fewer, the rest waits for a release
                    continue
                except BaseException as e:          # a bad request must not take the loop down: it fails alone
                    bad = group if len(group) == 1 else None
                    if bad is None:
                        group = group[:1]
                        continue
                    self._finish(bad[0], e)
                    with self._lock:
                        self._pending.remove(bad[0])
                    moved += 1
                    break
                with self._lock:
                    for r, s in zip(group, slots):
                        r.slot = s
                        self._active[s] = r
                        self._pending.remove(r)
                    self.max_concurrent = max(self.max_concurrent, len(self._active))
                moved += len(group)
                break
        return moved

    def _finish(self, req: _Request, error: Optional[BaseException] = None):
        req.error = error
        req.done.set()

    def _deliver(self):
        live, steps = self.engine.cb_poll()
        for s, req in list(self._active.items()):
            n = steps[s]
            if n > req.sent:
                toks = self.engine.cb_read(s, req.sent, n - req.sent)
                if req.lp is not None:              # before the tokens are handed over: a consumer that sees a token finds its record
                    req.lp_chunks.append(self.engine.cb_read_logprobs(s, req.sent, n - req.sent))
                req.chunks.append(toks)
                first, req.sent = req.sent, n
                if req.on_tokens is not None:
                    try:
                        req.on_tokens(toks, first)
                    except BaseException as e:      # the consumer failed: stop this request, keep the others
                        self.engine.cb_release(s)
                        del self._active[s]
                        self._finish(req, e)
                        continue
            if not live[s]:
                self.engine.cb_release(s)
                del self._active[s]
                self._finish(req)

    def _loop(self):
        try:
            if torch.cuda.is_available():
                torch.cuda.set_device(self.device)
        except Exception:
            pass
        try:
            while True:
                with self._lock:
                    while not self._pending and not self._active and not self._closing:
                        self._lock.wait()
                    if self._closing and not self._pending and not self._active:
                        break
                with self._lock:
                    head = self._pending[0] if self._pending else None
                try:
                    if head is not None and head.exclusive is not None:
                        if not self._active:        # the engine is idle: hand it over
                            with self._lock:
                                self._pending.popleft()
                            try:
                                self.engine.cb_reset()
                                head.value = head.exclusive()
                                self._finish(head)
                            except BaseException as e:
                                self._finish(head, e)
                            continue
                    elif self._pending and len(self._active) < self.slots:
                        moved = self._admit()
                        if moved == 0 and not self._active:
                            # nothing runs and the head request still does not fit: no release will ever make room.  Reset the
                            # continuous batch once (recovers anything a failed admit left behind); if it still does not fit,
                            # the request fails with an error instead of the loop spinning on it forever.
                            self.engine.cb_reset()
                            if self._admit() == 0:
                                with self._lock:
                                    head = self._pending.popleft() if self._pending else None
                                if head is not None:
                                    self._finish(head, StarVectorBusy(
                                        "the request does not fit an idle engine (KV pages / slots for prompt + max_new_tokens)"))
                                continue
                        self._deliver()             # first tokens (and one-token requests) right away
                    if self._active:
                        self.engine.cb_step(self.steps_per_poll)
                        self.steps_run += self.steps_per_poll
                        self._deliver()
                except Exception as e:              # the engine failed under this batch (a device error, a row of non-finite
                    with self._lock:                # logits): the requests SHARING the batch learn about it at once, the
                        reqs = list(self._active.values())      # waiting ones stay queued and the loop lives on -- one
                        self._active.clear()                    # poisoned request must not take the worker down
                    for r in reqs:
                        self._finish(r, e)
                    try:
                        self.engine.cb_reset()
                    except Exception:
                        pass
        except BaseException as e:                  # interpreter shutdown and the like: every request learns about it at once
            with self._lock:
                reqs = list(self._active.values()) + list(self._pending)
                self._active.clear()
                self._pending.clear()
                self._closing = True
            for r in reqs:
                self._finish(r, e)
        finally:
            try:
                self.engine.cb_reset()
            except Exception:
                pass
