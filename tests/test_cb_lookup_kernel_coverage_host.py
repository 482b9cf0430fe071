"""CPU: the kernels of csrc/cb_lookup/*.hip are accounted for the way tests/test_lookup_kernel_coverage_host.py accounts for
csrc/lookup/*.hip -- with tests/test_kernel_coverage_host.py's own parser and checker, over a table of their own: each kernel names a test
that holds it to a reference on caller-given rows and a test that reaches it through the engine -- and the three older tables still describe
exactly their directories."""
import os

from tests import test_kernel_coverage_host as T
from tests import test_lookup_kernel_coverage_host as TL
from tests import test_lookup_sampled_kernel_coverage_host as TS

OPS = "test_gpu_cb_lookup_ops.py::"
E2E = "test_gpu_cb_lookup.py::"

COVERAGE = {
    # held to the Python restatement whose chooser is the plain step's selection on the same row and state (cb_step_kernel through
    # sv_op_cb_select), then through the engine: all-right forced drafts fail when a row does not see its siblings' K / V or its slot's state
    "cb_lookup_step_kernel": (OPS + "test_one_launch_is_the_restatement", OPS + "test_eos_stop_stop_any_and_budget_inside_an_accepted_run",
                              E2E + "test_forced_drafts_right_partly_wrong_and_all_wrong", E2E + "test_logprob_records_are_the_plain_batchs_bit_for_bit"),
}


def _kernel_names(monkeypatch, sub):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, sub))               # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_cb_lookup_kernel_is_accounted_for(monkeypatch):
    names = _kernel_names(monkeypatch, "cb_lookup")
    assert len(names) == 1 and set(names.values()) == {"cb_lookup.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k, tests in COVERAGE.items():
        assert any(t.startswith(OPS) for t in tests) and any(t.startswith(E2E) for t in tests), k      # an op test and an engine test each
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k                  # deleting any one entry fails


def test_the_three_older_tables_still_see_exactly_their_directories(monkeypatch):
    new = _kernel_names(monkeypatch, "cb_lookup")
    sampled = _kernel_names(monkeypatch, "lookup_sampled")
    lookup = _kernel_names(monkeypatch, "lookup")
    old = T.kernel_names()
    assert not set(new) & (set(old) | set(lookup) | set(sampled)), "a cb_lookup kernel is visible to an older table"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)
    assert set(lookup) == set(TL.COVERAGE) and len(lookup) == 4 and not T.check_table(TL.COVERAGE, lookup)
    assert set(sampled) == set(TS.COVERAGE) and len(sampled) == 2 and not T.check_table(TS.COVERAGE, sampled)
