"""The keyframe database's entry points: declared, exported and built, and what they refuse without touching a device (no GPU)."""
import ctypes as C
import os

import numpy as np

from tests.helpers import ROOT

NAMES = ("slamit_kfdb_create", "slamit_kfdb_destroy", "slamit_kfdb_clear", "slamit_kfdb_info", "slamit_kfdb_add", "slamit_kfdb_add_dev",
         "slamit_kfdb_erase", "slamit_kfdb_query", "slamit_kfdb_query_batch_dev")


def test_kfdb_is_declared_exported_and_built():
    from weiner_slamit_v2_amd import api, build

    build.build()
    hdr = open(os.path.join(ROOT, "include", "slamit.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib(), name), name
    assert "kfdb.hip" in build.SOURCES and "kfdb.hip" not in build.PER_FILE   # the default flags: -ffp-contract=off is part of the numerics
    assert hasattr(api, "KeyFrameDatabase")


def test_too_many_words_per_slot_are_refused_before_any_device_call():
    from weiner_slamit_v2_amd import api

    L = api.lib()
    h = C.c_void_p()
    assert L.slamit_kfdb_create(10, api.VOC_MAX_FEATURES + 1, 0, C.byref(h)) == -1 and not h.value
    assert b"max_words > SLAMIT_VOC_MAX_FEATURES" in L.slamit_last_error()
    assert L.slamit_kfdb_create(0, 100, 0, C.byref(h)) == -1 and not h.value and b"at least 1" in L.slamit_last_error()


def test_unsorted_and_repeated_word_ids_are_refused_before_any_device_call():
    """A BowVector is a std::map: its word ids ascend strictly.  The host forms check the vector before they look at the handle."""
    from weiner_slamit_v2_amd import api

    L = api.lib()
    v = np.full(4, 0.25)
    slot = C.c_int32(-5)
    out_i, out_d = np.zeros(4, np.int32), np.zeros(4, np.float64)
    for words in ([3, 2, 5, 9], [1, 4, 4, 9], [-1, 0, 1, 2]):
        w = np.array(words, np.int32)
        assert L.slamit_kfdb_add(None, w.ctypes.data, v.ctypes.data, 4, C.byref(slot)) == -1
        assert b"slamit_kfdb_add: word ids are not strictly ascending" in L.slamit_last_error() and slot.value == -5
        assert L.slamit_kfdb_query(None, w.ctypes.data, v.ctypes.data, 4, out_i.ctypes.data, out_i.ctypes.data, None, out_d.ctypes.data) == -1
        assert b"slamit_kfdb_query: word ids are not strictly ascending" in L.slamit_last_error()
    good = np.array([1, 4, 6, 9], np.int32)
    assert L.slamit_kfdb_add(None, good.ctypes.data, v.ctypes.data, 4, C.byref(slot)) == -1 and b"null argument" in L.slamit_last_error()
    assert L.slamit_kfdb_erase(None, 0) == -1 and L.slamit_kfdb_clear(None) == -1 and L.slamit_kfdb_info(None, None, None, None) == -1
