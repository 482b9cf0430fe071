"""CPU: the kernels of csrc/kv8/*.hip are accounted for the way tests/test_kernel_coverage_host.py accounts for csrc/*.hip -- with that
file's own parser and checker, over a table of their own -- and the old table still describes exactly the old directory.  (The e4m3 forms
of kv_write_prefill_kernel and attn_decode_kernel are template arguments of names the old table holds; tests/test_gpu_kv_fp8_ops.py runs them.)"""
import os

from tests import test_kernel_coverage_host as T

OPS = "test_gpu_kv_fp8_ops.py::"
E2E = "test_gpu_kv_fp8.py::"

COVERAGE = {
    # both pool formats read back: the bf16 pool's stored bits, the e4m3 pool against the torch restatement of the rule bit for bit
    "kv_read_kernel": (OPS + "test_quantiser_read_back_is_the_restatement", OPS + "test_appended_row_is_the_restatement_of_the_steps_own_row",
                       E2E + "test_exactness_on_one_fp8_kv_engine"),
}


def _kv8_kernel_names(monkeypatch):
    monkeypatch.setattr(T, "CSRC", os.path.join(T.CSRC, "kv8"))            # kernel_names() globs CSRC/*.hip
    try:
        return T.kernel_names()
    finally:
        monkeypatch.undo()


def test_every_kv8_kernel_is_accounted_for(monkeypatch):
    names = _kv8_kernel_names(monkeypatch)
    assert len(names) == 1 and set(names.values()) == {"kv8.hip"}, names
    wrong = T.check_table(COVERAGE, names)
    assert not wrong, "\n".join(wrong)
    for k in COVERAGE:                                           # deleting any one entry fails
        assert T.check_table({a: b for a, b in COVERAGE.items() if a != k}, names), k


def test_the_old_table_still_sees_exactly_the_old_directory(monkeypatch):
    new = _kv8_kernel_names(monkeypatch)
    old = T.kernel_names()
    assert not set(new) & set(old), "a kv8 kernel is visible to csrc/*.hip"
    assert set(old) == set(T.COVERAGE) and not T.check_table(T.COVERAGE, old)


def test_the_e4m3_forms_are_template_arguments_of_the_old_names():
    """attention.hip grew no kernel name: the KV format is a template parameter of kv_write_prefill_kernel and attn_decode_kernel, and both
    instantiations of each are launched."""
    text = open(os.path.join(T.CSRC, "attention.hip")).read()
    assert "template <bool RAG, int KVF = 0>" in text and "template <int D, int NS, int KVF = 0>" in text
    for launch in ("kv_write_prefill_kernel<false, 1>", "kv_write_prefill_kernel<true, 1>", "launch_attn_decode_as<128, 4, 1>",
                   "launch_attn_decode_as<64, 8, 1>"):
        assert launch in text, launch
