"""The rectangle's band selector without a GPU: the symbols are exported and
the constants of drep_amd._lib equal the header's."""
import os
import re

from drep_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _defines():
    hdr = open(os.path.join(ROOT, "include", "drephip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(DREPHIP_[A-Z_]+)\s+(-?\d+)\b", hdr)}


def test_rect_band_symbols_are_exported():
    L = _lib.lib()
    for name in ("drephip_set_rect_band", "drephip_last_rect_info"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    # a null context is an argument error, not a crash
    assert L.drephip_set_rect_band(None, 0, 64) == -1
    assert L.drephip_last_rect_info(None, None, None) == -1


def test_rect_band_constants_equal_the_header():
    d = _defines()
    C = _lib.Context
    assert (C.RECT_BAND_AUTO, C.RECT_BAND_OFF, C.RECT_BAND_FORCE) == \
        (d["DREPHIP_RECT_BAND_AUTO"], d["DREPHIP_RECT_BAND_OFF"], d["DREPHIP_RECT_BAND_FORCE"]) == (0, 1, 2)
    # what drephip_last_rect_info reports
    assert (C.AP_AUTO, C.AP_TABLE, C.AP_BAND, C.AP_MERGE) == \
        (d["DREPHIP_AP_AUTO"], d["DREPHIP_AP_TABLE"], d["DREPHIP_AP_BAND"], d["DREPHIP_AP_MERGE"])
