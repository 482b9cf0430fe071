"""CPU: the kernels of csrc/mxfp4/*.hip are accounted for the way tests/test_kernel_coverage_host.py accounts for csrc/*.hip -- with that
file's own parser and checker, over a table of their own -- and the old table still describes exactly the old directory."""
import os

from tests import test_kernel_coverage_host as T

OPS = "test_gpu_mxfp4_ops.py::"
E2E = "test_gpu_mxfp4.py::"

COVERAGE = {
    # both images against the torch restatement of the format (exact, natural and designed rows, bf16 and fp32 sources), then through the engine
    "mxfp4_pack_kernel": (OPS + "test_quantiser_images_are_the_restatement_in_the_stated_layouts",
                          E2E + "test_against_the_oracle_over_the_fake_quantised_weights"),
    # the three output forms against float64 on dequant(quant(W)), every col_tiles value to the same bits, rows independent of the batch
    "gemm_skinny_mxfp4_kernel": (OPS + "test_decode_gemm_slabs_against_float64_on_the_dequantised_weights",
                                 OPS + "test_decode_gemm_epilogues_against_float64_on_the_dequantised_weights",
                                 OPS + "test_rows_do_not_depend_on_the_batch"),
}


def _mxfp4_kernel_names(monkeypatch):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, "mxfp4"))          # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_mxfp4_kernel_is_accounted_for(monkeypatch):
    names = _mxfp4_kernel_names(monkeypatch)
    assert len(names) == 2 and set(names.values()) == {"mxfp4.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k in COVERAGE:                                           # deleting any one entry fails
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k


def test_the_old_table_still_sees_exactly_the_old_directory(monkeypatch):
    new = _mxfp4_kernel_names(monkeypatch)
    old = T.kernel_names()
    assert not set(new) & set(old), "an mxfp4 kernel is visible to csrc/*.hip"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)
