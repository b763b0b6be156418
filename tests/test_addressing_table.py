"""The coverage table of tests/test_gpu_addressing.py, checked without a GPU: every *_dev method of jpezy_amd.api.Context that takes a
frame count or frames from a tensor's leading dimension has a row, and every cell names a test that exists or says why there is none."""
import test_gpu_addressing as TA


def test_every_batch_method_has_a_row():
    TA.check_table()


def test_a_missing_row_and_a_dangling_cell_are_noticed(monkeypatch):
    import pytest
    row = TA.COVERAGE["huffman_histogram_dev"]
    monkeypatch.delitem(TA.COVERAGE, "huffman_histogram_dev")
    with pytest.raises(AssertionError, match="methods without a row"):
        TA.check_table()
    monkeypatch.setitem(TA.COVERAGE, "huffman_histogram_dev", {"420": ("test_no_such_test[420]",) + row["420"][1:]})
    with pytest.raises(AssertionError, match="names no test of this module"):
        TA.check_table()
