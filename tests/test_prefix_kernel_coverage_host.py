"""CPU: the kernels of csrc/prefix/*.hip are accounted for the way tests/test_kernel_coverage_host.py accounts for csrc/*.hip -- with that
file's own parser and checker, over a table of their own -- and the old table still describes exactly the old directory."""
import os

from tests import test_kernel_coverage_host as T

GPU = "test_gpu_prefix_scoring.py::"

COVERAGE = {
    # (engine) a wrong position shows in every kept row of the learned-position model (wpe) and of the rotary one (RoPE): both contracts hold the
    # pass to the solo run's bits, prefixes of 5, 64 and 257 rows in one call
    "prefix_row_pos_kernel": (GPU + "test_forward_logprobs_prefixed_tiny_models_bitwise", GPU + "test_forward_logprobs_prefixed_sliding_window"),
}


def _prefix_kernel_names(monkeypatch):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, "prefix"))          # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_prefix_kernel_is_accounted_for(monkeypatch):
    names = _prefix_kernel_names(monkeypatch)
    assert len(names) == 1 and set(names.values()) == {"prefix.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k in COVERAGE:                                           # deleting any one entry fails
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k


def test_the_old_table_still_sees_exactly_the_old_directory(monkeypatch):
    new = _prefix_kernel_names(monkeypatch)
    old = T.kernel_names()
    assert not set(new) & set(old), "a prefix kernel is visible to csrc/*.hip"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)
