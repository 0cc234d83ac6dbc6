"""A text in host or device memory between guard bytes: the one `Mem` of every GPU test that hands the engine raw
pointers (tests/aead_batch_cases.py and the five files it serves, tests/test_gpu_eax_siv.py, tests/test_gpu_ff1.py,
tests/test_gpu_ff3.py, tests/test_gpu_kw.py, tests/test_gpu_kwp.py, tests/test_gpu_ocb.py, tests/test_gpu_siv_v.py)."""
import ctypes as C

GUARD, FILL, ROOM = 0xA5, 0x5C, 64


class Mem:
    """`size` bytes (starting with `data`, then `fill`) in host or device memory, `off` bytes behind a 4-byte-aligned
    address, with ROOM guard bytes on either side"""

    def __init__(self, data=b"", device=False, off=0, size=None, fill=FILL):
        data = bytes(data)
        self.size = max(len(data), size or 0)
        self.at, self.device, self.fill = ROOM + off, device, fill
        raw = bytes([GUARD]) * self.at + data + bytes([fill]) * (self.size - len(data)) + bytes([GUARD]) * (ROOM + 4)
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

    def intact(self, n=None):
        """nothing outside the `size` bytes was written; with n: nor anything but the first n of them"""
        r = self.raw()
        rest = set() if n is None else set(r[self.at + n:self.at + self.size])
        return set(r[:self.at]) | set(r[self.at + self.size:]) == {GUARD} and rest <= {self.fill}


def ptr(x):
    """what a C entry point takes for an array that is bytes, None or Mem"""
    return x.ptr if isinstance(x, Mem) else x
