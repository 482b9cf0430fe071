"""CPU: the kernels of csrc/prefix_cache/*.hip are accounted for the way tests/test_kernel_coverage_host.py accounts for csrc/*.hip -- with
that file's own parser and checker, over a table of their own -- and the old table still describes exactly the old directory."""
import os

from tests import test_kernel_coverage_host as T

OPS = "test_gpu_prefix_cache_ops.py::"
E2E = "test_gpu_prefix_cache.py::"

COVERAGE = {
    # the digests against the numpy restatement bit for bit, both forms; the engine's lookups stand on them
    "page_digest_kernel": (OPS + "test_digests_are_the_restatement_bit_for_bit", OPS + "test_offset_and_neighbours_do_not_enter",
                           OPS + "test_one_bit_and_one_swap_change_exactly_their_page", OPS + "test_the_rectangular_form_equals_the_ragged_form",
                           E2E + "test_shared_prefix_reuses_exactly_the_common_full_pages"),
}


def _pc_kernel_names(monkeypatch):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, "prefix_cache"))   # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_prefix_cache_kernel_is_accounted_for(monkeypatch):
    names = _pc_kernel_names(monkeypatch)
    assert len(names) == 1 and set(names.values()) == {"prefix_cache.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k in COVERAGE:                                           # deleting any one entry fails
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k


def test_the_old_table_still_sees_exactly_the_old_directory(monkeypatch):
    new = _pc_kernel_names(monkeypatch)
    old = T.kernel_names()
    assert not set(new) & set(old), "a prefix-cache kernel is visible to csrc/*.hip"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)


def test_the_source_is_built_into_the_library():
    from starvector_amd import build
    assert os.path.join("prefix_cache", "prefix_cache.hip") in build.SOURCES
