"""The rectangle's two-set screen without a GPU: the symbols are exported, the
constants of drep_amd._lib equal the header's, the mode argument is checked
before anything touches a device, and DREPHIP_RECT_SCREEN's parser reads the
three words as context creation does."""
import ctypes as C
import os
import re

import pytest

from drep_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


def _defines():
    hdr = open(os.path.join(ROOT, "include", "drephip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define\s+(DREPHIP_[A-Z_]+)\s+(-?\d+)\b", hdr)}


def test_rect_screen_symbols_are_exported():
    L = _lib.lib()
    for name in ("drephip_set_rect_screen", "drephip_last_rect_screen_stats", "drephip_last_rect_screen_ms",
                 "drephip_rect_screen_mode_of"):
        assert name in _lib.SIGNATURES
        assert getattr(L, name) is not None
    # a null context is an argument error, not a crash
    assert L.drephip_set_rect_screen(None, 0) == ERR_ARG
    assert L.drephip_last_rect_screen_stats(None, None, None, None, None, None, None, None) == ERR_ARG
    assert L.drephip_last_rect_screen_ms(None, None) == ERR_ARG


def test_rect_screen_constants_equal_the_header():
    d = _defines()
    Ctx = _lib.Context
    assert (Ctx.RECT_SCREEN_AUTO, Ctx.RECT_SCREEN_OFF, Ctx.RECT_SCREEN_FORCE) == \
        (d["DREPHIP_RECT_SCREEN_AUTO"], d["DREPHIP_RECT_SCREEN_OFF"], d["DREPHIP_RECT_SCREEN_FORCE"]) == (0, 1, 2)
    assert callable(Ctx.set_rect_screen) and callable(Ctx.last_rect_screen_stats)


@pytest.mark.parametrize("text,mode", [("auto", 0), ("off", 1), ("force", 2), ("", 0), ("OFF", 0), ("forced", 0),
                                       ("1", 0)])
def test_rect_screen_environment_words(text, mode):
    """What a new context makes of DREPHIP_RECT_SCREEN: the three words, and
    auto for anything else (as DREPHIP_RECT_BAND reads its own)."""
    L = _lib.lib()
    m = C.c_int(77)
    assert L.drephip_rect_screen_mode_of(text.encode(), C.byref(m)) == 0
    assert m.value == mode


def test_rect_screen_parser_checks_its_arguments():
    L = _lib.lib()
    m = C.c_int(77)
    assert L.drephip_rect_screen_mode_of(None, C.byref(m)) == ERR_ARG
    assert L.drephip_rect_screen_mode_of(b"off", None) == ERR_ARG
    assert m.value == 77


def test_the_screen_is_part_of_the_library():
    """rect_screen.hip is built into libdrephip.so (Makefile OBJS) and counted
    in the source digest."""
    mk = open(os.path.join(ROOT, "drep_amd", "csrc", "Makefile")).read()
    assert "$(OUT)/rect_screen.o" in mk
    assert os.path.exists(os.path.join(ROOT, "drep_amd", "csrc", "rect_screen.hip"))
