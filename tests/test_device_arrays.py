"""tests/device_arrays.py itself: the guard check every device test relies on (split_guarded, on the CPU), and on the GPU the round
trips of Guarded, upload, upload_records and raw.  No library call: the writes beside an output are torch writes into the tensor
the helper owns."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.device_arrays import GUARD, SENTINEL, UNTOUCHED, Guarded, raw, split_guarded, upload, upload_records


def _buffer(inside, guard_bytes):
    b = np.ascontiguousarray(inside).view(np.uint8).reshape(-1)
    return np.concatenate([np.full(guard_bytes, SENTINEL, np.uint8), b, np.full(guard_bytes, SENTINEL, np.uint8)])


# ------------------------------------------------------------------ CPU
def test_split_guarded_returns_the_inside_of_an_intact_buffer():
    inside = np.arange(40, dtype=np.int32) - 7
    inside[3] = np.int32(-1515870811)  # four SENTINEL bytes inside the array are data
    got = split_guarded(_buffer(inside, 128), 128, inside.nbytes)
    assert got.dtype == np.uint8 and np.array_equal(got.view(np.int32), inside)


@pytest.mark.parametrize("at", ["front first", "front last", "back first", "back last"])
def test_split_guarded_raises_for_one_changed_guard_byte(at):
    inside = np.full(10, UNTOUCHED, np.int32)
    g = 4 * GUARD
    buf = _buffer(inside, g)
    buf[{"front first": 0, "front last": g - 1, "back first": g + inside.nbytes, "back last": len(buf) - 1}[at]] ^= 1
    with pytest.raises(AssertionError, match="a guard .* was written"):
        split_guarded(buf, g, inside.nbytes)


def test_split_guarded_of_an_empty_inside_still_checks_both_guards():
    buf = _buffer(np.zeros(0, np.int32), 64)
    assert len(buf) == 128 and split_guarded(buf, 64, 0).size == 0
    for at in (0, 63, 64, 127):
        bad = buf.copy()
        bad[at] = 0
        with pytest.raises(AssertionError, match="a guard .* was written"):
            split_guarded(bad, 64, 0)


def test_split_guarded_with_rows_of_28_bytes():
    assert O.KP_DTYPE.itemsize == 28
    keys = np.zeros(5, O.KP_DTYPE)
    keys["x"], keys["octave"] = np.arange(5), 3
    g = GUARD * 28
    buf = _buffer(keys, g)
    assert np.array_equal(split_guarded(buf, g, keys.nbytes).view(O.KP_DTYPE), keys)
    buf[g + keys.nbytes] = 0  # the first byte of the row behind the last record
    with pytest.raises(AssertionError, match="a guard .* was written"):
        split_guarded(buf, g, keys.nbytes)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_guarded_round_trip_and_a_write_on_either_side():
    import torch
    initial = (np.arange(15, dtype=np.float32) * np.float32(0.37) - 2).reshape(5, 3)
    for cell in (None, -1, initial.size):  # untouched; the cell just before the array; the cell just behind it
        g = Guarded(initial)
        assert g.guard_bytes == GUARD * 12 and g.ptr == g.t.data_ptr() + g.guard_bytes and g.view.shape == (5, 3)
        if cell is None:
            got = g.fetch()
            assert got.dtype == np.float32 and got.shape == (5, 3) and np.array_equal(got.view(np.uint8), initial.view(np.uint8))
            assert g.untouched()
            g.view[4, 2] = 1.0  # a write inside: no guard complains, and the array is no longer untouched
            assert g.fetch()[4, 2] == 1.0 and not g.untouched()
            continue
        g.t.view(torch.float32)[g.guard_bytes // 4 + cell] = 0.0
        torch.cuda.synchronize()
        with pytest.raises(AssertionError, match="a guard .* was written"):
            g.fetch()
        assert not g.untouched()
    empty = Guarded(np.zeros((0, 3), np.float32))
    assert empty.t.numel() == 2 * GUARD * 12 and empty.fetch().shape == (0, 3) and empty.untouched()
    cells = Guarded.cells(7)
    assert cells.fetch().dtype == np.int32 and (cells.fetch() == UNTOUCHED).all() and bool((cells.view == UNTOUCHED).all())


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [False, True])
def test_gpu_upload_with_front_and_pad_entries(fill):
    a = np.zeros(9, O.KP_DTYPE)
    a["x"], a["class_id"] = np.arange(9) + 0.5, -1
    t, address = upload(a, front=64, pad=64, fill=a[4] if fill else None)
    edges = (a[4:5] if fill else np.zeros(1, O.KP_DTYPE)).tobytes() * 64
    assert t.numel() == (64 + 9 + 64) * 28 and address == t.data_ptr() + 64 * 28
    assert np.array_equal(raw(address, a.nbytes).cpu().numpy().view(O.KP_DTYPE), a)
    assert raw(address - 64 * 28, 64 * 28).cpu().numpy().tobytes() == edges and raw(address + a.nbytes, 64 * 28).cpu().numpy().tobytes() == edges
    rows = np.arange(12, dtype=np.float32).reshape(4, 3)  # an entry is a row
    t, address = upload(rows, front=64, pad=64)
    assert t.numel() == (64 + 4 + 64) * 12 and np.array_equal(raw(address, 48).cpu().numpy().view(np.float32).reshape(4, 3), rows)


@pytest.mark.gpu
def test_gpu_bare_upload_is_typed_and_an_empty_array_gives_an_empty_tensor():
    import torch
    t, address = upload(np.arange(6, dtype=np.int32).reshape(2, 3))
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 3) and address == t.data_ptr()
    assert np.array_equal(raw(address, 24).cpu().numpy().view(np.int32), np.arange(6))
    assert upload(np.zeros(0, np.float32))[0].numel() == 0
    assert upload(np.arange(3, dtype=np.uint32))[0].dtype == torch.uint8  # bytes, as for a record dtype
    assert upload(np.zeros(2, O.KP_DTYPE))[0].numel() == 56


@pytest.mark.gpu
def test_gpu_upload_records_reads_back_byte_identical():
    class Record(C.Structure):
        _fields_ = [("p", C.c_void_p * 5), ("f", C.c_float * 4), ("n", C.c_int), ("flag", C.c_int)]

    assert C.sizeof(Record) == 64
    recs = [Record((C.c_void_p * 5)(*[0x7f0000000000 + 256 * (5 * i + j) for j in range(5)]), (C.c_float * 4)(i, 0.5, -1.5, 1e-3), 100 + i, i % 2) for i in range(3)]
    t = upload_records(recs)
    assert t.numel() == 192
    assert raw(t.data_ptr(), 192).cpu().numpy().tobytes() == b"".join(bytes(r) for r in recs)
