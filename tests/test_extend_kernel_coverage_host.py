"""CPU: the kernels of csrc/extend/*.hip are accounted for the way tests/test_kernel_coverage_host.py accounts for csrc/*.hip -- with that
file's own parser and checker, over a table of their own -- and the old table still describes exactly the old directory.  (The attention of an
extension pass is the prefixed form of attn_prefill_kernel, a name the old table holds; tests/test_gpu_extend_ops.py runs it over the cache.)"""
import os

from tests import test_kernel_coverage_host as T

OPS = "test_gpu_extend_ops.py::"
CHUNK = "test_gpu_chunked_prefill.py::"

COVERAGE = {
    # both pool formats against sv_debug_kv_read bit for bit (and, for the bf16 pool, against the rows that were stored); then as the attention's
    # operand: a wrong gathered row changes the logits and pages the contract tests compare
    "kv_gather_kernel": (OPS + "test_kv_gather_is_kv_read_bit_for_bit", OPS + "test_contract_a_open_and_extends_equal_the_one_shot_ragged_pass",
                         OPS + "test_contract_b_e4m3_cache_is_exact_against_a_bf16_twin"),
    # held to the BITS of kv_write_prefill_kernel's pages (the one-shot pass), cached tokens untouched, zero tail; e4m3: against tests/kv8_ref.py
    "kv_write_extend_kernel": (OPS + "test_writer_keeps_cached_tokens_and_writes_own_rows_as_the_one_shot_writer",
                               OPS + "test_contract_b_e4m3_cache_is_exact_against_a_bf16_twin",
                               CHUNK + "test_prefill_and_generate_return_the_same_under_a_budget"),
}


def _extend_kernel_names(monkeypatch):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, "extend"))          # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_extend_kernel_is_accounted_for(monkeypatch):
    names = _extend_kernel_names(monkeypatch)
    assert len(names) == 2 and set(names.values()) == {"extend.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k in COVERAGE:                                           # deleting any one entry fails
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k


def test_the_old_table_still_sees_exactly_the_old_directory(monkeypatch):
    new = _extend_kernel_names(monkeypatch)
    old = T.kernel_names()
    assert not set(new) & set(old), "an extend kernel is visible to csrc/*.hip"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)
