"""The general-shape mode's wide-path switch (fs_set_general_wide_rows) and pass counter
(fs_general_wide_passes): process-wide host state that makes no HIP call, so it is
checked here without a GPU."""
from flowstate import _lib


def test_general_wide_rows_setter_and_counter():
    L = _lib.load()
    passes = L.fs_general_wide_passes()
    assert passes >= 0
    start = L.fs_set_general_wide_rows(-1)  # a negative argument only reads
    assert 0 <= start <= 65536
    assert L.fs_set_general_wide_rows(-7) == start
    try:
        assert L.fs_set_general_wide_rows(1000) == start  # returns the previous value
        assert L.fs_set_general_wide_rows(-1) == 1000
        assert L.fs_set_general_wide_rows(1 << 40) == 1000
        assert L.fs_set_general_wide_rows(-1) == 65536  # capped
        assert L.fs_set_general_wide_rows(0) == 65536
        assert L.fs_set_general_wide_rows(-1) == 0  # 0 disables, and is not a read
    finally:
        L.fs_set_general_wide_rows(start)
    assert L.fs_set_general_wide_rows(-1) == start  # restored
    assert L.fs_general_wide_passes() == passes  # no pass was launched


def test_default_mode_limit_is_untouched():
    L = _lib.load()
    wide = L.fs_set_wide_rows(12345)
    try:
        prev = L.fs_set_general_wide_rows(77)
        try:
            assert L.fs_set_wide_rows(12345) == 12345
        finally:
            L.fs_set_general_wide_rows(prev)
    finally:
        L.fs_set_wide_rows(wide)
