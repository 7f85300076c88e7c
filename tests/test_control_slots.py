"""CPU side of the device control path (rift_control_tick): the (env_id, cbv_id) -> controller-state row map and the ctypes mirror of
RiftControlCBV."""
import ctypes

from rift_amd.planning.pluto.inference import ControlSlots


def test_new_keys_get_distinct_rows_and_keep_them():
    s = ControlSlots()
    a, b, c = s.slot((0, 5)), s.slot((0, 6)), s.slot((1, 5))
    assert sorted((a, b, c)) == [0, 1, 2]                       # never-used rows, handed out in order (they hold zeros)
    assert (s.slot((0, 5)), s.slot((0, 6)), s.slot((1, 5))) == (a, b, c)
    assert (0, 5) in s and (2, 5) not in s and len(s) == 3 and s.rows == 3
    assert sorted(s.keys()) == [(0, 5), (0, 6), (1, 5)]


def test_a_released_row_is_reused_only_after_it_was_zeroed():
    s = ControlSlots()
    a, b = s.slot((0, 1)), s.slot((0, 2))
    s.release((0, 1))
    assert (0, 1) not in s and s.pending() == [a]
    c = s.slot((0, 3))                                           # the released row still holds the old controller: a new row instead
    assert c not in (a, b) and s.rows == 3 and s.pending() == [a]
    s.zeroed(s.pending())
    assert s.pending() == []
    d = s.slot((0, 4))                                           # zeroed: handed out again, no new row
    assert d == a and s.rows == 3
    assert s.slot((0, 1)) == 3                                   # the CBV that left comes back as a new one: fresh row, not its old state
    s.release((9, 9))                                            # unknown key: nothing happens
    assert s.pending() == []


def test_release_and_reuse_of_several_rows():
    s = ControlSlots()
    rows = [s.slot((0, k)) for k in range(6)]
    for k in (1, 3, 4):
        s.release((0, k))
    assert sorted(s.pending()) == [rows[1], rows[3], rows[4]]
    s.zeroed([rows[3]])                                          # a partial confirmation frees exactly those rows
    assert sorted(s.pending()) == [rows[1], rows[4]]
    assert s.slot((1, 0)) == rows[3]
    assert s.slot((1, 1)) == 6
    live = [s.slot(k) for k in s.keys()]
    assert len(set(live)) == len(live) and not set(live) & set(s.pending())


def test_ctypes_mirror_of_the_descriptor():
    from rift_amd import _ffi
    st = _ffi.RiftControlCBV
    assert ctypes.sizeof(st) == 40
    assert [getattr(st, f).offset for f, *_ in st._fields_] == [0, 4, 8, 16, 24, 32]
    assert [f for f, *_ in st._fields_] == ["batch_index", "slot", "x", "y", "heading", "speed"]
    assert "rift_control_tick" in _ffi.EXPORTS and _ffi.CONTROL_STATE == 44
