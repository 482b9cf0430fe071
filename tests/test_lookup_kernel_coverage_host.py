"""CPU: the kernels of csrc/lookup/*.hip are accounted for the way tests/test_kernel_coverage_host.py accounts for csrc/*.hip -- with that
file's own parser and checker, over a table of their own -- and the old table still describes exactly the old directory."""
import os

from tests import test_kernel_coverage_host as T

OPS = "test_gpu_lookup_ops.py::"
E2E = "test_gpu_lookup.py::"

COVERAGE = {
    # held to the BITS of attn_decode_kernel's own append (K1 sequential launches against one launch behind the pre-write), then through the engine
    "lookup_kv_write_kernel": (OPS + "test_prewrite_gives_the_bits_of_sequential_decode", E2E + "test_forced_drafts_right_partly_wrong_and_all_wrong"),
    "lookup_hold_eos_kernel": (OPS + "test_min_length_hold_per_row", E2E + "test_natural_lookup_equals_the_plain_call_on_the_goldens"),
    "lookup_step_kernel": (OPS + "test_accept_against_the_restatement", OPS + "test_draft_against_the_restatement"),
    # (engine) the first drafts and the row layout: a wrong one changes the step counts of the forced-draft tests and the ragged positions
    "lookup_begin_kernel": (E2E + "test_forced_drafts_right_partly_wrong_and_all_wrong", E2E + "test_ragged_prompts"),
}


def _lookup_kernel_names(monkeypatch):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, "lookup"))          # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_lookup_kernel_is_accounted_for(monkeypatch):
    names = _lookup_kernel_names(monkeypatch)
    assert len(names) == 4 and set(names.values()) == {"lookup.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k in COVERAGE:                                           # deleting any one entry fails
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k


def test_the_old_table_still_sees_exactly_the_old_directory(monkeypatch):
    new = _lookup_kernel_names(monkeypatch)
    old = T.kernel_names()
    assert not set(new) & set(old), "a lookup kernel is visible to csrc/*.hip"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)
