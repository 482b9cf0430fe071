"""CPU: the kernels of csrc/lookup_sampled/*.hip are accounted for the way tests/test_lookup_kernel_coverage_host.py accounts for
csrc/lookup/*.hip -- with tests/test_kernel_coverage_host.py's own parser and checker, over a table of their own -- and the two older
tables still describe exactly their directories."""
import os

from tests import test_kernel_coverage_host as T
from tests import test_lookup_kernel_coverage_host as TL

OPS = "test_gpu_lookup_sampled_ops.py::"
E2E = "test_gpu_lookup_sampled.py::"

COVERAGE = {
    # held to the BITS of sample_top_p_kernel row by row (same device code, the plain call's (seed, step, row) triple), then through the engine
    "lookup_sample_kernel": (OPS + "test_every_row_draws_what_the_plain_sampler_draws_at_its_column", E2E + "test_forced_drafts_right_partly_wrong_and_all_wrong"),
    # held to a Python set model, then through the engine: all-right forced drafts under a penalty fail when a row misses a draft in front of it
    "lookup_seen_kernel": (OPS + "test_seen_sets_against_the_set_model", E2E + "test_forced_drafts_right_partly_wrong_and_all_wrong"),
}


def _kernel_names(monkeypatch, sub):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, sub))               # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_sampled_lookup_kernel_is_accounted_for(monkeypatch):
    names = _kernel_names(monkeypatch, "lookup_sampled")
    assert len(names) == 2 and set(names.values()) == {"lookup_sampled.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k in COVERAGE:                                           # deleting any one entry fails
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k


def test_the_two_older_tables_still_see_exactly_their_directories(monkeypatch):
    new = _kernel_names(monkeypatch, "lookup_sampled")
    lookup = _kernel_names(monkeypatch, "lookup")
    old = T.kernel_names()
    assert not set(new) & set(old) and not set(new) & set(lookup), "a sampled-lookup kernel is visible to an older table"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)
    assert set(lookup) == set(TL.COVERAGE) and len(lookup) == 4 and not T.check_table(TL.COVERAGE, lookup)
