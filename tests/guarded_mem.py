"""A text in host or device memory between guard bytes, for the GPU tests that hand the engine raw pointers
(tests/test_gpu_kw.py, tests/test_gpu_kwp.py)."""
import ctypes as C

GUARD, FILL, ROOM = 0xA5, 0x5C, 64


class Mem:
    """`size` bytes (starting with `data`, then FILL) in host or device memory, `off` bytes behind a 4-byte-aligned
    address, with ROOM guard bytes on either side"""

    def __init__(self, data=b"", device=False, off=0, size=None):
        data = bytes(data)
        self.size = max(len(data), size or 0)
        self.at, self.device = ROOM + off, device
        raw = bytes([GUARD]) * self.at + data + bytes([FILL]) * (self.size - len(data)) + bytes([GUARD]) * (ROOM + 4)
        if device:
            import torch
            self.t = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to("cuda")
            base = self.t.data_ptr()
        else:
            self.h = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
            base = C.addressof(self.h)
        assert base % 4 == 0
        self.ptr = C.c_void_p(base + self.at)

    def raw(self):
        if self.device:
            import torch
            torch.cuda.synchronize()
            return bytes(self.t.cpu().numpy())
        return bytes(self.h)

    def get(self, n=None):
        return self.raw()[self.at:self.at + (self.size if n is None else n)]

    def intact(self):
        """nothing outside the `size` bytes was written"""
        r = self.raw()
        return set(r[:self.at]) | set(r[self.at + self.size:]) == {GUARD}
