"""The handle checks every entry point starts with (csrc/pa_api.cpp: check_index,
begin_align) answer before any HIP call, so they are tested without a GPU: a
NULL index is PA_EINVAL with the text "NULL argument" from each of them."""

import ctypes

import pytest

import pa_native as N

_DUMMY = ctypes.create_string_buffer(64)

NULL_INDEX_CALLS = {
    "pa_index_prepare": lambda L: L.pa_index_prepare(None, None),
    "pa_index_prepare_ex": lambda L: L.pa_index_prepare_ex(None, 1, None),
    "pa_index_prepare_coverage": lambda L: L.pa_index_prepare_coverage(None, None),
    "pa_index_reduce": lambda L: L.pa_index_reduce(None, None, 0, 0, None),
    "pa_result_create": lambda L: L.pa_result_create(None, ctypes.byref(N.P())),
    "pa_coverage_create": lambda L: L.pa_coverage_create(None, ctypes.byref(N.P())),
    "pa_pileup_create": lambda L: L.pa_pileup_create(None, ctypes.byref(N.P())),
    "pa_abundance_create": lambda L: L.pa_abundance_create(None, ctypes.byref(N.P())),
    "pa_align_reads": lambda L: L.pa_align_reads(None, None, ctypes.byref(N.Params.make()), ctypes.byref(N.U64()),
                                                 None, None, ctypes.byref(N.U64()), None, 0,
                                                 ctypes.byref(N.U64()), None),
    # (reads and acc not NULL, and never read: the index is looked at first)
    "pa_coverage_add": lambda L: L.pa_coverage_add(None, ctypes.addressof(_DUMMY), ctypes.byref(N.Params.make()),
                                                   ctypes.addressof(_DUMMY), None),
}


@pytest.mark.parametrize("name", sorted(NULL_INDEX_CALLS))
def test_null_index_is_einval(name):
    L = N.lib()
    assert NULL_INDEX_CALLS[name](L) == N.PA_EINVAL
    assert L.pa_last_error() == b"NULL argument"
