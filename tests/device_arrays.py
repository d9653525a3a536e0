"""Device arrays of the GPU tests and of tools/bench_matchers.py: what every device-resident entry point's test needs around its own
fields.  Inputs are uploaded with readable entries before and behind the payload, so a kernel that follows a wrong index reads inside
the test's own allocation and shows as a wrong result or status; outputs lie between guard rows of a byte sentinel, so a kernel that
writes beside its output is seen by the next fetch().  No debugger and no device sanitizer stands behind these tests: the guards are
the evidence.  tests/test_device_arrays.py tests this module.

Device memory is torch tensors; torch is imported inside the functions, so collecting the CPU tests needs no GPU."""
import ctypes as C
import gc
import time
import types

import numpy as np

UNTOUCHED = -7                          # what int32 output cells hold before a call (as float bits: a NaN no weight sum can be)
HAS_UNTOUCHED, XW_UNTOUCHED = 9, -7.0   # the same for has_point bytes and Xw floats
BEYOND = 1 << 30                        # what cur_point holds at and beyond a frame's keypoint count: never a keypoint's, never written
SENTINEL = 0xA5                         # every byte of a guard row
GUARD = 32                              # guard rows before and behind an output


def raw(ptr, nbytes):
    """A raw device pointer as a zero-copy torch uint8 tensor."""
    import torch
    iface = {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}
    return torch.as_tensor(types.SimpleNamespace(__cuda_array_interface__=iface), device="cuda:0")


def _row_bytes(a):
    return a.dtype.itemsize * int(np.prod(a.shape[1:], dtype=np.int64))


def upload(a, front=0, pad=0, fill=None):
    """`front` entries, the payload, `pad` entries in HBM (zeros, or copies of the entry `fill`); returns the tensor that owns the
    memory and the payload's address.  Without front and pad the tensor is typed and shaped as `a` (bytes for a record dtype or
    uint32), and an empty array gives an empty tensor: pass `t.data_ptr() if t.numel() else 0` where the library is to see NULL."""
    import torch
    a = np.ascontiguousarray(a)
    if not front and not pad:
        if a.dtype.fields or a.dtype == np.uint32:
            a = a.view(np.uint8).reshape(-1)
        t = torch.from_numpy(a.copy()).to("cuda:0")
        return t, t.data_ptr()
    edge = lambda k: np.zeros((k,) + a.shape[1:], a.dtype) if fill is None else np.repeat(np.asarray([fill], a.dtype), k, axis=0)
    whole = np.concatenate([edge(front), a, edge(pad)])
    t = torch.from_numpy(whole.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    return t, t.data_ptr() + front * _row_bytes(a)


def upload_records(recs):
    """A sequence of ctypes structures of one type as device bytes."""
    recs = list(recs)
    return upload(np.frombuffer(bytes((type(recs[0]) * len(recs))(*recs)), np.uint8))[0]


def split_guarded(raw_bytes, guard_bytes, inside_bytes):
    """The inside of a fetched guarded buffer (uint8); AssertionError if any guard byte no longer holds SENTINEL."""
    raw_bytes = np.asarray(raw_bytes)
    assert raw_bytes.dtype == np.uint8 and raw_bytes.shape == (2 * guard_bytes + inside_bytes,)
    end = guard_bytes + inside_bytes
    before, behind = np.nonzero(raw_bytes[:guard_bytes] != SENTINEL)[0], np.nonzero(raw_bytes[end:] != SENTINEL)[0]
    if before.size or behind.size:
        raise AssertionError("a guard byte was written: %d bytes before the array (from its start: %s), %d behind it (from its end: %s)" % (
            before.size, (before - guard_bytes)[:8].tolist(), behind.size, behind[:8].tolist()))
    return raw_bytes[guard_bytes:end]


class Guarded:
    """An array the device writes, starting out as `initial`, between `guard_rows` rows of SENTINEL bytes on either side (a row is
    initial[0]'s size).  ptr is the array's address; view is the array as a torch tensor, for work queued on a stream."""

    def __init__(self, initial, guard_rows=GUARD):
        import torch
        a = np.ascontiguousarray(initial)
        self.dtype, self.shape, self.nbytes, self.guard_bytes = a.dtype, a.shape, a.nbytes, guard_rows * _row_bytes(a)
        self.whole = np.full(2 * self.guard_bytes + a.nbytes, SENTINEL, np.uint8)
        self.whole[self.guard_bytes: self.guard_bytes + a.nbytes] = a.view(np.uint8).reshape(-1)
        self.t = torch.from_numpy(self.whole).to("cuda:0")
        self.ptr = self.t.data_ptr() + self.guard_bytes

    @classmethod
    def cells(cls, n, value=UNTOUCHED):
        """n int32 cells of `value`."""
        return cls(np.full(n, value, np.int32))

    @property
    def view(self):
        import torch
        inside = self.t[self.guard_bytes: self.guard_bytes + self.nbytes]
        return inside.view(torch.from_numpy(np.empty(0, self.dtype)).dtype).view(self.shape)

    def fetch(self):
        """The array as the device left it; asserts that both guards are intact."""
        return split_guarded(self.t.cpu().numpy(), self.guard_bytes, self.nbytes).view(self.dtype).reshape(self.shape).copy()

    def untouched(self):
        """Guards intact and the array still equal to `initial`, byte for byte."""
        return np.array_equal(self.t.cpu().numpy(), self.whole)


def context(api, **kw):
    """A context with the camera of tests/test_matchers.py."""
    from tests import test_matchers as TM
    return api.Context(width=TM.W, height=TM.H, fx=TM.FX, fy=TM.FY, cx=TM.CX, cy=TM.CY, bf=TM.BF, **kw)


def device_buffers(ctx):
    """The addresses of the context's own device buffers (orbfe_device_buffers)."""
    p = [C.c_void_p() for _ in range(5)]
    ctx._check(ctx.L.orbfe_device_buffers(ctx.h, *[C.byref(x) for x in p]))
    return dict(kps=p[0].value, desc=p[1].value, counts=p[2].value, u_right=p[3].value)


def timed_loops(fn, reps):
    """(mean, slowest) in ms of `reps` calls of fn after one warm-up call, each timed on its own: one stalled call shows as such.
    The cyclic garbage collector is off inside the window, as in the standard timeit module."""
    fn()
    gc.collect()
    gc.disable()
    try:
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            t.append((time.perf_counter() - t0) * 1e3)
    finally:
        gc.enable()
    return round(sum(t) / reps, 4), round(max(t), 4)
